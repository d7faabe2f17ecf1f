"""The conv_igemm builds that read their weight fragments from the packed tensor (csrc/conv_igemm.hip, conv_direct_a: the
exact fp32 128 x 128 builds of the 3x3 kernel and of the 1x1 kernel with 16-channel chunks, POST twin and grouped launch
included) held to the bits of builds that stage their weights through LDS.

Every exact build adds an output's products in the order chunk -> tap -> quad pair -> element, so a row of a large launch
(128 x 128 tiles) must equal the same row of a launch small enough for the launcher to take 32-pixel tiles.  Each case first
asks the launcher (ops.conv2d_plan) which build every launch takes, so that no build is compared with itself, and also
holds the large launch to float64 (tolerances.assert_close_via_f64).  The packed weights lie at the front of a larger
NaN-filled buffer: a fragment read past the tensor that reached an MFMA would show.  Sources of 3, 1, 2 and 12 channels end
in ragged chunks (zero rows of the pack inside a quad pair, skipped quad pairs in the 1x1 build); 130 couts (160 packed)
make the second cout tile clamp its rows.

The 1x1 builds have the path switched off (DM_CONV_DIRECT_A in the kernel source: they measured slower with it); their
cases hold whichever loop the library was built with."""
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

KEYS = ('KS', 'WGM', 'WGN', 'WM', 'WN', 'CK', 'TAIL', 'PREC', 'POST')
B128, B32 = (3, 2, 2, 2, 2, 8, 0, 0, 0), (3, 4, 1, 1, 1, 8, 0, 0, 0)
P128, PSMALL = (1, 2, 2, 2, 2, 16, 0, 0, 0), (1, 4, 1, 1, 1, 32, 0, 0, 0)
P128_POST, PSMALL_POST = P128[:8] + (1,), PSMALL[:8] + (1,)
NAN_TAIL = 1 << 16


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _builds(ops, srcs, NB, H, W, cout, ks, **kw):
    return [(tuple(r[k] for k in KEYS), r['MAXPOS']) for r in ops.conv2d_plan(srcs, NB, H, W, cout, ks, **kw)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _problem(ops, srcs, NB, H, W, cout, ks, seed):
    cin = sum(srcs)
    w = torch.randn(cout, cin, ks, ks, generator=_g(seed)) / (cin * ks * ks) ** 0.5
    b = torch.randn(cout, generator=_g(seed + 1))
    xs = [torch.randn(NB, c, H, W, generator=_g(seed + 2 + i)) for i, c in enumerate(srcs)]
    wq = ops.pack_conv_weight(w.cuda(), src_channels=list(srcs))
    big = torch.full((wq.numel() + NAN_TAIL,), float('nan'), device='cuda')
    big[:wq.numel()] = wq
    return dict(w=w, b=b, xs=xs, xs_dev=[t.cuda() for t in xs], b_dev=b.cuda(), wq=big[:wq.numel()])


def _small_chunk(ops, srcs, H, W, cout, ks, small, most=58, **kw):
    """The largest batch of at most `most` RoIs whose launch is one launch of the build `small`."""
    for n in range(most, 0, -1):
        if _builds(ops, srcs, n, H, W, cout, ks, **kw) == [small]:
            return n
    raise AssertionError(f'no batch of at most {most} RoIs takes {small}')


def _in_chunks(NB, step, fn):
    return torch.cat([fn(i, min(i + step, NB)) for i in range(0, NB, step)])


def _f64(p, idx, ks, relu=False, prev=None, mask=None, addend=None):
    x = torch.cat([t[idx] for t in p['xs']], 1)
    r32 = F.conv2d(x, p['w'], p['b'], padding=ks // 2)
    r64 = F.conv2d(x.double(), p['w'].double(), p['b'].double(), padding=ks // 2)
    if prev is not None:
        r32, r64 = r32 + prev[idx], r64 + prev[idx].double()
    if relu:
        r32, r64 = r32.relu(), r64.relu()
    if addend is not None:
        r32, r64 = r32 + addend[idx], r64 + addend[idx].double()
    if mask is not None:
        r32, r64 = torch.where(mask[idx] > 0, r32, torch.zeros(())), torch.where(mask[idx] > 0, r64, torch.zeros((), dtype=torch.float64))
    return r32, r64


def _sample(NB, step):
    idx = {0, 1, NB - 2, NB - 1} | {i for s in range(step, NB, step) for i in (s - 1, s)}
    return sorted(i for i in idx if 0 <= i < NB)[:12]


# ------------------------------------------------------------------ 3x3
VARIANTS = ('relu', 'accumulate', 'mask')


def _run3(ops, p, lo, hi, cout, variant, prev, mask, overlapped=False):
    xs = [t[lo:hi].contiguous() for t in p['xs_dev']]
    kw = {}
    out = None
    if variant == 'relu':
        kw['relu'] = True
    if variant == 'accumulate':
        out = prev[lo:hi].cuda()
        kw['accumulate'] = True
    if variant == 'mask':
        kw['mask'] = mask[lo:hi].cuda()
    if overlapped:
        with ops.overlapped_streams():
            return ops.conv2d(xs, p['wq'], p['b_dev'], cout, 3, out=out, **kw)
    return ops.conv2d(xs, p['wq'], p['b_dev'], cout, 3, out=out, **kw)


def _plan_kw(variant):
    return dict(relu=variant == 'relu', accumulate=variant == 'accumulate', has_mask=variant == 'mask')


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cout', [256, 250, 130])
@pytest.mark.parametrize('srcs', [[8], [12], [8, 3, 1]], ids=lambda s: 'x'.join(map(str, s)))
def test_3x3_14_rows_equal_the_32_pixel_build(ops, srcs, cout, variant):
    H = W = 14
    NBS = (59, 122)
    NB = max(NBS)
    pk = _plan_kw(variant)
    for n in NBS:
        assert _builds(ops, srcs, n, H, W, cout, 3, **pk) == [(B128, 1)]
    step = _small_chunk(ops, srcs, H, W, cout, 3, (B32, 1), **pk)
    p = _problem(ops, srcs, NB, H, W, cout, 3, seed=hash((tuple(srcs), cout)) % 1000)
    prev = torch.randn(NB, cout, H, W, generator=_g(7)) if variant == 'accumulate' else None
    mask = torch.randn(NB, cout, H, W, generator=_g(8)) if variant == 'mask' else None
    ref = _in_chunks(NB, step, lambda lo, hi: _run3(ops, p, lo, hi, cout, variant, prev, mask))
    for n in NBS:
        out = _run3(ops, p, 0, n, cout, variant, prev, mask)
        assert torch.equal(out, ref[:n]), f'NB {n}: rows differ from the 128 x 32 build\'s'
    idx = _sample(NB, step)
    r32, r64 = _f64(p, idx, 3, relu=variant == 'relu', prev=prev, mask=mask)
    assert_close_via_f64(ref[idx].cpu(), r32, r64, f'3x3 {srcs} -> {cout} {variant}')


def test_3x3_14_seam_and_overlapped(ops):
    srcs, cout, H, W, NB = [8], 256, 14, 14, 512
    main_tail = _builds(ops, srcs, NB, H, W, cout, 3, relu=True)
    assert main_tail == [(B128, 1), (B32, 1)]
    assert _builds(ops, srcs, NB, H, W, cout, 3, relu=True, overlapped=True) == [(B128, 1)]
    step = _small_chunk(ops, srcs, H, W, cout, 3, (B32, 1), relu=True)
    p = _problem(ops, srcs, NB, H, W, cout, 3, seed=31)
    ref = _in_chunks(NB, step, lambda lo, hi: _run3(ops, p, lo, hi, cout, 'relu', None, None))
    assert torch.equal(_run3(ops, p, 0, NB, cout, 'relu', None, None), ref), 'main + tail'
    assert torch.equal(_run3(ops, p, 0, NB, cout, 'relu', None, None, overlapped=True), ref), 'overlapped: one launch'
    idx = _sample(NB, 128)
    r32, r64 = _f64(p, idx, 3, relu=True)
    assert_close_via_f64(ref[idx].cpu(), r32, r64, '3x3 seam')


def test_3x3_28_two_positions_per_thread(ops):
    srcs, cout, H, W, NB = [8, 3, 1], 130, 28, 28, 67
    assert _builds(ops, srcs, NB, H, W, cout, 3) == [(B128, 2)]
    step = _small_chunk(ops, srcs, H, W, cout, 3, (B32, 1))
    p = _problem(ops, srcs, NB, H, W, cout, 3, seed=41)
    ref = _in_chunks(NB, step, lambda lo, hi: _run3(ops, p, lo, hi, cout, 'plain', None, None))
    assert torch.equal(_run3(ops, p, 0, NB, cout, 'plain', None, None), ref)
    idx = _sample(NB, step)
    r32, r64 = _f64(p, idx, 3)
    assert_close_via_f64(ref[idx].cpu(), r32, r64, '3x3 28 x 28')


def test_3x3_group_launch(ops):
    # three problems of 59 RoIs fill the chip: the grouped 128 x 128 build; each problem has the bits of its own small launches
    cin, cout, H, W, NB = 12, 130, 14, 14, 59
    step = _small_chunk(ops, [cin], H, W, cout, 3, (B32, 1), relu=True)
    ps = [_problem(ops, [cin], NB, H, W, cout, 3, seed=50 + 5 * i) for i in range(3)]
    outs = ops.conv2d_group([p['xs_dev'][0] for p in ps], [p['wq'] for p in ps], [p['b_dev'] for p in ps], cout, 3, relu=True, split=False)
    for i, p in enumerate(ps):
        ref = _in_chunks(NB, step, lambda lo, hi: _run3(ops, p, lo, hi, cout, 'relu', None, None))
        assert torch.equal(outs[i], ref), f'problem {i}'
        idx = _sample(NB, step)
        r32, r64 = _f64(p, idx, 3, relu=True)
        assert_close_via_f64(outs[i][idx].cpu(), r32, r64, f'3x3 group problem {i}')


# ------------------------------------------------------------------ 1x1
SRCS1 = [[16], [24, 8, 1, 1], [16, 16, 2]]


def _run1(ops, p, lo, hi, cout, addend=None):
    xs = [t[lo:hi].contiguous() for t in p['xs_dev']]
    if addend is not None:
        return ops.conv1x1_post_add(xs, p['wq'], p['b_dev'], cout, addend[lo:hi].cuda(), relu=True)
    return ops.conv2d(xs, p['wq'], p['b_dev'], cout, 1, relu=True)


@pytest.mark.parametrize('post', [False, True], ids=['plain', 'post_add'])
@pytest.mark.parametrize('cout', [256, 130])
@pytest.mark.parametrize('srcs', SRCS1, ids=lambda s: 'x'.join(map(str, s)))
def test_1x1_14_rows_equal_the_32_pixel_build(ops, srcs, cout, post):
    H, W, NB = 14, 14, 105
    big, small = (P128_POST, PSMALL_POST) if post else (P128, PSMALL)
    pk = dict(relu=True, has_addend=post)
    assert _builds(ops, srcs, NB, H, W, cout, 1, **pk) == [(big, 1)]
    step = _small_chunk(ops, srcs, H, W, cout, 1, (small, 1), most=104, **pk)
    p = _problem(ops, srcs, NB, H, W, cout, 1, seed=hash((tuple(srcs), cout)) % 1000 + 1)
    addend = torch.randn(NB, cout, H, W, generator=_g(9)) if post else None
    ref = _in_chunks(NB, step, lambda lo, hi: _run1(ops, p, lo, hi, cout, addend))
    assert torch.equal(_run1(ops, p, 0, NB, cout, addend), ref), 'rows differ from the 128 x 32 build\'s'
    idx = _sample(NB, step)
    r32, r64 = _f64(p, idx, 1, relu=True, addend=addend)
    assert_close_via_f64(ref[idx].cpu(), r32, r64, f'1x1 {srcs} -> {cout} post {post}')


def test_1x1_group_launch(ops):
    # dm_conv2d_group_fwd takes the 128 x 128 build for more than 64 couts whatever the batch; 24 channels: a full chunk and
    # one of 8 channels, whose second quad pair is skipped
    cin, cout, H, W, NB = 24, 130, 14, 14, 20
    assert _builds(ops, [cin], NB, H, W, cout, 1, relu=True) == [(PSMALL, 1)]
    ps = [_problem(ops, [cin], NB, H, W, cout, 1, seed=70 + 5 * i) for i in range(2)]
    outs = ops.conv2d_group([p['xs_dev'][0] for p in ps], [p['wq'] for p in ps], [p['b_dev'] for p in ps], cout, 1, relu=True)
    for i, p in enumerate(ps):
        assert torch.equal(outs[i], _run1(ops, p, 0, NB, cout)), f'problem {i}'
        idx = list(range(NB))
        r32, r64 = _f64(p, idx, 1, relu=True)
        assert_close_via_f64(outs[i].cpu(), r32, r64, f'1x1 group problem {i}')
