"""Res2Net inference on the device: the sliced 3x3 kernel (dm_conv3x3_slices_fwd) against torch's CPU convolution of the
slices in float32 and float64, its tail, slice isolation with NaN and Inf, batch independence; the 2x2 ceil-mode average
pool and the deep stem's first convolution against torch; the argument checks of all three; ``backbones.Res2Net`` against
the reference's own module (tests/golden/g31_res2net.npz) and, stage by stage, against res2net_inputs.restate; the launch
count, host waits, and the chain through the detector."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the sliced kernel
WIDTHS = [6, 8, 26, 52, 104, 208]
# The kernel's output tile (csrc/conv_slices.hip) is 32 columns wide and 32 rows high for w <= 8, 8 rows high above, at
# both strides; a wave makes 8 output channels, a workgroup 8 (w <= 8) or 32; K is walked in chunks of 8 channels (2 in
# the 32-row build at stride 2); a lane stores 4 neighbouring columns, as one float4 where Wo % 4 == 0.  Of the issue's
# maps
#   (3, 37, 53) at stride 1 crosses every row edge (37 > 32) and the column edge (53 = 32 + 21); at stride 2 (19 x 27) the
#               row edges of the 8-row tiles;
#   (1, 5, 130) has 5 tile columns at stride 1 and 3 at stride 2 (65 = 2 * 32 + 1); (1, 3, 340) stores float4s at stride 1;
# and the added
#   (1, 67, 40) crosses the 32-row edge at stride 2 too (34 rows = 32 + 2), which no map of the issue's list does, and
#               takes the float4 stores at both strides (Wo = 40 and Wo = 20).
# The widths cross the channel edges: 6 < 8 = one chunk and one cout tile, 26 = 3 * 8 + 2 (a short last chunk, a cout tile
# with 2 live channels), 52 (7 cout tiles: a workgroup whose last wave has none), 104 and 208 (multiples of 8).
MAPS = [(1, 1, 1), (1, 2, 3), (2, 10, 14), (3, 37, 53), (1, 5, 130), (1, 3, 340), (1, 67, 40)]


def _offsets(w, G):
    """(x_ch0, a_ch0, o_ch0) inside 4w-channel tensors: non-zero, different from each other, no multiples of w."""
    return (2 * w + 1, w - 1, 3 * w - 2) if G == 1 else (w - 1, 1, w - 3 if w > 3 else 1)


def _problem(NB, w, G, H, W, seed):
    x = torch.randn(NB, 4 * w, H, W, generator=_g(seed))
    a = torch.randn(NB, 4 * w, H, W, generator=_g(seed + 1))
    wt = torch.randn(G, w, w, 3, 3, generator=_g(seed + 2)) * (2.0 / (9 * w)) ** 0.5
    b = torch.randn(G * w, generator=_g(seed + 3)) * 0.5
    return x, a, wt, b


def _ref(x, a, wt, b, w, G, stride, x_ch0, a_ch0, relu, dtype):
    """The slices' convolutions by torch on the CPU: [NB, G * w, Ho, Wo]."""
    outs = []
    for g in range(G):
        s = x[:, x_ch0 + g * w: x_ch0 + (g + 1) * w].to(dtype)
        if a is not None:
            s = s + a[:, a_ch0 + g * w: a_ch0 + (g + 1) * w].to(dtype)
        y = F.conv2d(s.contiguous(), wt[g].to(dtype), b[g * w:(g + 1) * w].to(dtype) if b is not None else None, stride, 1)
        outs.append(F.relu(y) if relu else y)
    return torch.cat(outs, 1)


@pytest.mark.parametrize('w', WIDTHS)
def test_conv3x3_slices_against_torch(w):
    from dynamask_amd import ops
    for G in (1, 3):
        x_ch0, a_ch0, o_ch0 = _offsets(w, G)
        for NB, H, W in MAPS:
            x, a, wt, b = _problem(NB, w, G, H, W, 3100 + 100 * H + W + w + G)
            xd, ad, bd = x.cuda(), a.cuda(), b.cuda()
            wq = ops.pack_conv_slices_weight(wt.cuda())
            small = NB * H * W <= 300
            for stride in (1, 2):
                assert ops.conv3x3_slices_supported(x, w, G, stride)
                Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
                for with_a in (False, True):
                    for relu, bias in ([(True, True), (False, False), (True, False), (False, True)] if small else [(True, True), (False, False)]):
                        args = (x, a if with_a else None, wt, b if bias else None, w, G, stride, x_ch0, a_ch0, relu)
                        ref32, ref64 = _ref(*args, torch.float32), _ref(*args, torch.float64)
                        out = torch.full((NB, 4 * w, Ho, Wo), NAN).cuda()
                        sentinel = _bits(out).clone()
                        kw = dict(stride=stride, relu=relu, x_ch0=x_ch0, o_ch0=o_ch0, addend=ad if with_a else None, a_ch0=a_ch0)
                        assert ops.conv3x3_slices(xd, wq, bd if bias else None, w, G, out, **kw) is out
                        name = f'conv3x3_slices w={w} G={G} {(NB, H, W)} stride={stride} relu={relu} bias={bias} addend={with_a}'
                        got = out[:, o_ch0:o_ch0 + G * w]
                        assert tuple(got.shape) == tuple(ref32.shape), name
                        err, ref_err, scale = assert_close_via_f64(got, ref32, ref64, name)
                        print(f'{name}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
                        keep = [c for c in range(4 * w) if not o_ch0 <= c < o_ch0 + G * w]
                        assert torch.equal(_bits(out)[:, keep], sentinel[:, keep]), name + ': a channel outside the slices was written'
                        again = torch.full_like(out, NAN)
                        ops.conv3x3_slices(xd, wq, bd if bias else None, w, G, again, **kw)
                        assert torch.equal(_bits(again), _bits(out)), name + ': a second call gives other bits'
            assert torch.equal(xd.cpu(), x) and torch.equal(ad.cpu(), a), 'x or addend was written'


@pytest.mark.parametrize('w,G', [(6, 1), (6, 3), (26, 1), (26, 3)], ids=lambda v: str(v))
def test_tail_copies_or_pools_in_the_same_launch(w, G):
    """Mode 1: the source's bits.  Mode 2: AvgPool2d(3, stride, padding=1) with the divisor 9, odd sizes included.  The
    slices' outputs have the bits of the launch without a tail, and nothing else of ``out`` is written."""
    from dynamask_amd import ops
    C = (G + 2) * w
    x_ch0, o_ch0, tail_x, tail_o = w, 0, 0, (G + 1) * w - 1          # the tail reads in front of the slices, writes behind
    for NB, H, W in [(1, 1, 1), (1, 2, 3), (2, 10, 14), (3, 37, 53)]:
        x = torch.randn(NB, C, H, W, generator=_g(3300 + H + w))
        wt = torch.randn(G, w, w, 3, 3, generator=_g(3301)) * (2.0 / (9 * w)) ** 0.5
        xd, wq = x.cuda(), ops.pack_conv_slices_weight(wt.cuda())
        src = x[:, tail_x:tail_x + w]
        for stride, tail in ((1, 1), (1, 2), (2, 2)):
            Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
            plain = ops.conv3x3_slices(xd, wq, None, w, G, torch.full((NB, C, Ho, Wo), NAN).cuda(), stride=stride, relu=True, x_ch0=x_ch0,
                                       o_ch0=o_ch0)
            out = torch.full((NB, C, Ho, Wo), NAN).cuda()
            ops.conv3x3_slices(xd, wq, None, w, G, out, stride=stride, relu=True, x_ch0=x_ch0, o_ch0=o_ch0, tail=tail, tail_x_ch0=tail_x,
                               tail_o_ch0=tail_o)
            name = f'tail={tail} w={w} G={G} {(NB, H, W)} stride={stride}'
            got = out[:, tail_o:tail_o + w].cpu()
            if tail == 1:
                assert torch.equal(_bits(got), _bits(src)), name
            else:
                ref32, ref64 = F.avg_pool2d(src, 3, stride, 1), F.avg_pool2d(src.double(), 3, stride, 1)
                assert_close_via_f64(got, ref32, ref64, name)
            rest = [c for c in range(C) if not tail_o <= c < tail_o + w]
            assert torch.equal(_bits(out)[:, rest], _bits(plain)[:, rest]), name + ': the slices or the untouched channels differ'
            assert bool(torch.isnan(plain[:, G * w:]).all()) and bool(torch.isfinite(plain[:, :G * w]).all()), name
        assert torch.equal(xd.cpu(), x)


@pytest.mark.parametrize('w', [6, 26])
def test_a_nan_or_an_inf_stays_in_its_slice(w):
    """One NaN, then one +Inf, at one pixel of one channel of slice 1 of 3 -- in ``x``, then in ``addend``: the outputs of
    slices 0 and 2 keep the clean run's bits (no product with another slice's input is formed, not even by zero), the
    poisoned slice has torch's pattern."""
    from nonfinite_cases import assert_same_nonfinite
    from dynamask_amd import ops
    G, H, W = 3, 7, 9
    x_ch0, a_ch0, o_ch0 = _offsets(w, G)
    x, a, wt, b = _problem(1, w, G, H, W, 3400 + w)
    wq, bd = ops.pack_conv_slices_weight(wt.cuda()), b.cuda()
    others = list(range(0, w)) + list(range(2 * w, 3 * w))
    own = list(range(w, 2 * w))

    def run(xs, as_, stride):
        out = torch.full((1, 4 * w, (H + stride - 1) // stride, (W + stride - 1) // stride), NAN).cuda()
        ops.conv3x3_slices(xs.cuda(), wq, bd, w, G, out, stride=stride, relu=True, x_ch0=x_ch0, o_ch0=o_ch0, addend=as_.cuda(), a_ch0=a_ch0)
        return out[:, o_ch0:o_ch0 + G * w].cpu()
    for stride in (1, 2):
        clean = run(x, a, stride)
        assert bool(torch.isfinite(clean).all())
        for special in (NAN, float('inf')):
            for through in ('x', 'addend'):
                xs, as_ = x.clone(), a.clone()
                if through == 'x':
                    xs[0, x_ch0 + w + w // 2, 2, 4] = special                # (an even row and column: a centre tap at stride 2)
                else:
                    as_[0, a_ch0 + w + w // 2, 2, 4] = special
                got = run(xs, as_, stride)
                name = f'w={w} stride={stride} special={special} through {through}'
                assert torch.equal(_bits(got[:, others]), _bits(clean[:, others])), name + ': another slice changed'
                args = (xs, as_, wt, b, w, G, stride, x_ch0, a_ch0, True)
                ref32, ref64 = _ref(*args, torch.float32), _ref(*args, torch.float64)
                assert torch.equal(torch.isnan(got), torch.isnan(ref32)), name + ': isnan pattern'
                assert bool(torch.isfinite(ref32[:, others]).all()), name
                if special != special:       # every window over the pixel, in every output channel of the slice
                    assert int(torch.isnan(got[:, own]).sum()) == int(torch.isnan(got).sum()) == w * (9 if stride == 1 else 1), name
                else:
                    assert_same_nonfinite(got, ref32, ref64, name)


@pytest.mark.parametrize('w,G', [(8, 3), (26, 1), (26, 3), (52, 3)], ids=lambda v: str(v))
def test_slices_image_bits_do_not_depend_on_the_batch(w, G):
    from dynamask_amd import ops
    x_ch0, a_ch0, o_ch0 = _offsets(w, G)
    x, a, wt, b = _problem(3, w, G, 37, 53, 3500 + w)
    xd, ad, bd, wq = x.cuda(), a.cuda(), b.cuda(), ops.pack_conv_slices_weight(wt.cuda())
    for stride in (1, 2):
        kw = dict(stride=stride, relu=True, x_ch0=x_ch0, o_ch0=o_ch0, a_ch0=a_ch0, tail=2, tail_x_ch0=0, tail_o_ch0=0 if G == 1 else 4 * w - w)
        if G == 3:
            kw.update(o_ch0=0)
        shape = (4 * w, (37 + stride - 1) // stride, (53 + stride - 1) // stride)
        batch = ops.conv3x3_slices(xd, wq, bd, w, G, torch.zeros((3,) + shape).cuda(), addend=ad, **kw)
        for i in range(3):
            alone = ops.conv3x3_slices(xd[i:i + 1].contiguous(), wq, bd, w, G, torch.zeros((1,) + shape).cuda(), addend=ad[i:i + 1].contiguous(), **kw)
            assert torch.equal(_bits(alone[0]), _bits(batch[i])), f'stride {stride}, image {i}'


# ------------------------------------------------------------------------------------------------ the two small kernels
@pytest.mark.parametrize('H,W', [(1, 1), (2, 2), (3, 5), (37, 53)])
def test_avgpool2x2_ceil_against_torch(H, W):
    from dynamask_amd import ops
    x = torch.randn(2, 5, H, W, generator=_g(3600 + H))
    pool = lambda t: F.avg_pool2d(t, 2, 2, ceil_mode=True, count_include_pad=False)  # noqa: E731
    got = ops.avgpool2x2_ceil(x.cuda())
    assert tuple(got.shape) == (2, 5, (H + 1) // 2, (W + 1) // 2) == tuple(pool(x).shape)
    assert_close_via_f64(got, pool(x), pool(x.double()), f'avgpool2x2_ceil {(H, W)}')
    out = torch.full_like(got, NAN)
    assert ops.avgpool2x2_ceil(x.cuda(), out=out) is out and torch.equal(_bits(out), _bits(got))
    xs = x.clone()
    xs[1, 3, H - 1, W - 1] = NAN                 # the last element: alone in its window where H and W are odd
    xs[0, 2, 0, 0] = NAN
    got = ops.avgpool2x2_ceil(xs.cuda()).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(pool(xs))) and int(torch.isnan(got).sum()) == 2


@pytest.mark.parametrize('cout', [32, 37])
def test_conv3x3_s2_c3_against_torch(cout):
    """37 = 32 + 4 + 1 crosses the workgroup's 32 couts and its groups of 4."""
    from dynamask_amd import ops
    for NB, H, W in [(1, 1, 1), (2, 37, 53), (1, 6, 130)]:
        x = torch.randn(NB, 3, H, W, generator=_g(3700 + H))
        w = torch.randn(cout, 3, 3, 3, generator=_g(3701)) * (2.0 / 27) ** 0.5
        b = torch.randn(cout, generator=_g(3702)) * 0.5
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        assert ops.conv3x3_s2_c3_supported(x, cout)
        for relu, bias in ((True, True), (False, False)):
            act = F.relu if relu else (lambda t: t)
            ref32 = act(F.conv2d(x, w, b if bias else None, 2, 1))
            ref64 = act(F.conv2d(x.double(), w.double(), b.double() if bias else None, 2, 1))
            got = ops.conv3x3_s2_c3(xd, wd, bd if bias else None, relu=relu)
            name = f'conv3x3_s2_c3 cout={cout} {(NB, H, W)} relu={relu} bias={bias}'
            assert tuple(got.shape) == (NB, cout, (H + 1) // 2, (W + 1) // 2) == tuple(ref32.shape), name
            assert_close_via_f64(got, ref32, ref64, name)
            out = torch.full_like(got, NAN)
            assert ops.conv3x3_s2_c3(xd, wd, bd if bias else None, relu=relu, out=out) is out and torch.equal(_bits(out), _bits(got)), name
        assert torch.equal(xd.cpu(), x)
        if H > 2:       # a NaN pixel poisons exactly torch's outputs: every window over it, in every cout, through the ReLU
            xs = x.clone()
            xs[0, 1, 3, 5] = NAN
            got = ops.conv3x3_s2_c3(xs.cuda(), wd, bd, relu=True).cpu()
            ref = F.relu(F.conv2d(xs, w, b, 2, 1))
            assert torch.equal(torch.isnan(got), torch.isnan(ref)) and int(torch.isnan(got).sum()) == 4 * cout


def test_argument_checks():
    from dynamask_amd import _lib, ops
    L = _lib.lib()
    w, G = 6, 3
    x, a, wt, b = _problem(1, w, G, 9, 11, 3800)
    xd, ad, wq = x.cuda(), a.cuda(), ops.pack_conv_slices_weight(wt.cuda())
    out = torch.empty(1, 4 * w, 9, 11).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(xp=xd, ap=None, wp=wq, op=out, Cx=24, x0=0, Ca=24, a0=0, Co=24, o0=0, w=w, G=G, stride=1, flags=0, NB=1, tail=0, tx=18, to=18,
             H=9, W=11):
        return L.dm_conv3x3_slices_fwd(p(xp), Cx, x0, p(ap), Ca, a0, NB, w, G, H, W, stride, p(wp), None, flags, p(op), Co, o0, tail, tx, to, None)
    assert call() == 0 and call(ap=ad) == 0 and call(tail=1) == 0 and call(tail=2) == 0
    assert call(flags=1) == 0 and call(flags=8) == 0 and call(flags=9) == 0
    assert call(flags=16) == -3 and call(flags=17) == -3                  # bf16x3: unsupported
    assert call(flags=2) == -1 and call(flags=4) == -1 and call(flags=32) == -1 and call(flags=1 << 20) == -1
    assert call(xp=None) == -1 and call(wp=None) == -1 and call(op=None) == -1
    assert call(stride=3) == -1 and call(stride=0) == -1
    # slices that leave Cx / Ca / Co, negative offsets
    assert call(x0=7) == -1 and call(x0=-1) == -1 and call(o0=7) == -1 and call(o0=-1) == -1
    assert call(ap=ad, a0=7) == -1 and call(ap=ad, a0=-1) == -1 and call(ap=ad, Ca=17) == -1 and call(a0=7) == 0      # (no addend: unread)
    assert call(x0=6) == 0 and call(o0=6) == 0 and call(ap=ad, a0=6) == 0
    # the tail's ranges, and a tail that would write a slice's channels
    assert call(tail=1, tx=19) == -1 and call(tail=1, to=19) == -1 and call(tail=1, to=17) == -1 and call(tail=2, tx=-1) == -1
    assert call(tail=1, to=0, o0=6) == 0
    # what dm_conv3x3_slices_supported refuses, dm_conv3x3_slices_fwd refuses as unsupported
    for kw in (dict(w=0), dict(G=0), dict(H=0), dict(W=0), dict(tail=3), dict(tail=-1), dict(stride=2, tail=1), dict(Cx=17), dict(Co=17),
               dict(Co=18, tail=1), dict(NB=-1)):
        full = dict(NB=1, w=w, G=G, H=9, W=11, stride=1, Cx=24, Co=24, tail=0)
        full.update(kw)
        assert L.dm_conv3x3_slices_supported(*(full[k] for k in ('NB', 'w', 'G', 'H', 'W', 'stride', 'Cx', 'Co', 'tail'))) == 0, kw
        assert call(**kw) == -3, kw
    assert call(NB=0, xp=None, wp=None, op=None) == 0                      # nothing to do
    # the wrapper
    marked = wq.clone()
    marked._dm_bf16x3 = True               # what pack_conv_weight(precision='bf16x3') marks its result with
    with pytest.raises(RuntimeError, match='dm_conv3x3_slices_fwd'):
        ops.conv3x3_slices(xd, marked, None, w, G, out)
    with pytest.raises(AssertionError):
        ops.conv3x3_slices(xd, wq, None, w, 2, out)
    with pytest.raises(AssertionError):
        ops.conv3x3_slices(xd, wq, None, w, G, out, stride=2)
    with pytest.raises(NotImplementedError, match='stride=3'):
        ops.conv3x3_slices(xd, wq, None, w, G, out, stride=3)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.conv3x3_slices(x, wq, None, w, G, out)
    with pytest.raises(RuntimeError, match='dm_conv3x3_slices_fwd'):
        ops.conv3x3_slices(xd, wq, None, w, G, out, x_ch0=7)
    # the small kernels
    pin, pout = torch.zeros(4, 9, 11).cuda(), torch.zeros(4, 5, 6).cuda()
    assert L.dm_avgpool2x2_ceil_fwd(p(pin), 4, 9, 11, p(pout), None) == 0
    assert L.dm_avgpool2x2_ceil_fwd(None, 4, 9, 11, p(pout), None) == -1 and L.dm_avgpool2x2_ceil_fwd(p(pin), 4, 9, 11, None, None) == -1
    assert L.dm_avgpool2x2_ceil_supported(4, 0, 11) == 0 and L.dm_avgpool2x2_ceil_fwd(p(pin), 4, 0, 11, p(pout), None) == -3
    assert L.dm_avgpool2x2_ceil_supported(-1, 9, 11) == 0 and L.dm_avgpool2x2_ceil_fwd(p(pin), -1, 9, 11, p(pout), None) == -3
    assert L.dm_avgpool2x2_ceil_fwd(None, 0, 9, 11, None, None) == 0
    img, w3, o3 = torch.zeros(1, 3, 9, 11).cuda(), torch.zeros(32, 3, 3, 3).cuda(), torch.zeros(1, 32, 5, 6).cuda()

    def c3(xp=img, wp=w3, op=o3, NB=1, C=3, H=9, W=11, cout=32, flags=0):
        return L.dm_conv3x3_s2_c3_fwd(p(xp), NB, C, H, W, p(wp), None, cout, flags, p(op), None)
    assert c3() == 0 and c3(flags=1) == 0 and c3(flags=9) == 0
    assert c3(flags=16) == -3 and c3(flags=2) == -1 and c3(xp=None) == -1 and c3(wp=None) == -1 and c3(op=None) == -1
    for kw in (dict(C=4), dict(NB=0), dict(H=0), dict(cout=0)):
        full = dict(NB=1, C=3, H=9, W=11, cout=32)
        full.update(kw)
        assert L.dm_conv3x3_s2_c3_supported(*(full[k] for k in ('NB', 'C', 'H', 'W', 'cout'))) == 0 and c3(**kw) == -3, kw
    with pytest.raises(ValueError, match='conv3x3_s2_c3'):
        ops.conv3x3_s2_c3(img, torch.zeros(32, 4, 3, 3).cuda(), None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the module
@pytest.fixture(scope='module')
def net(golden_dir):
    """(Res2Net on the device with seeded weights, the seeded state, the backbone config, res2net_inputs, the fixture's
    images on the device)."""
    import res2net_inputs as xi
    from dynamask_amd import backbones, registry
    with open(os.path.join(golden_dir, xi.CONFIGS)) as f:
        cfg = json.load(f)[xi.RUN]['model']['backbone']
    m = registry.build_backbone(copy.deepcopy(cfg))
    assert type(m) is backbones.Res2Net
    state = xi.head_state({k: v.shape for k, v in m.state_dict().items()}, xi.WEIGHT_SEED)
    assert list(state) == sorted(xi.state_shapes(cfg))
    m.load_state_dict(state, strict=True)
    return m.cuda().eval(), state, cfg, xi, xi.inputs().cuda()


def test_forward_against_the_reference(net, golden_dir):
    from dynamask_amd import conv_precision
    m, _, cfg, xi, img = net
    z = np.load(os.path.join(golden_dir, xi.FILE))
    before = img.clone()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
        with conv_precision('bf16x3'):
            outs3 = m(img)
    assert torch.equal(_bits(img), _bits(before)), 'forward wrote into its input'
    assert isinstance(outs, tuple) and len(outs) == 4
    for l, (got, second, other) in enumerate(zip(outs, again, outs3)):
        ref32 = z[f'r2_101_out{l}']
        assert tuple(got.shape) == ref32.shape, f'output {l}'
        err, ref_err, scale = assert_close_via_f64(got, ref32, xi.unpack_f64(ref32, z[f'r2_101_out{l}_err16']), f'output {l}')
        print(f'r2_101 output {l}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
        assert torch.equal(_bits(got), _bits(second)), f'output {l}: a second call gives other bits'
        assert torch.equal(_bits(got), _bits(other)), f'output {l}: the bf16x3 mode changed the backbone'


def test_stem_and_every_stage_on_the_references_input(net):
    """The stem and every stage on the float32 restatement's own input to it: an error shows at the part that makes it."""
    m, state, cfg, xi, img = net
    with torch.no_grad():
        stem32, stages32 = xi.restate(cfg, state, xi.inputs(), every_stage=True)
        stem64 = xi.restate_stem(state, xi.inputs().double())
        got = m.stem(img)
        assert_close_via_f64(got, stem32, stem64, 'stem')
        x = stem32
        for i, ref32 in enumerate(stages32):
            ref64 = xi.restate_stage(cfg, state, i, x.double())
            xd = x.cuda()
            keep = xd.clone()
            got = m.run_stage(i, xd)
            assert torch.equal(_bits(xd), _bits(keep)), f'stage {i} wrote into its input'
            err, ref_err, scale = assert_close_via_f64(got, ref32, ref64, f'stage {i}')
            print(f'stage {i}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
            x = ref32


def test_launches_host_waits_and_batch_independence(net, monkeypatch):
    import bench
    from dynamask_amd import ops
    m, _, _, _, img = net
    before = img.clone()
    with torch.no_grad():
        both = m(img)
        alone = m(img[:1].contiguous())
        assert bench.count_host_syncs(lambda: m(img)) == 0
    assert torch.equal(_bits(img), _bits(before)), 'forward wrote into its input'
    for l, (a, b) in enumerate(zip(alone, both)):
        assert torch.equal(_bits(a[0]), _bits(b[0])), f'output {l}: an image\'s bits depend on the batch'
    calls = []
    for fn in ('conv2d', 'conv3x3_slices', 'avgpool2x2_ceil', 'conv3x3_s2_c3', 'conv3x3_dil', 'maxpool3x3_s2'):
        def counted(*a, _real=getattr(ops, fn), _fn=fn, **k):
            calls.append((_fn, k.get('stride', 1), a[4] if _fn == 'conv3x3_slices' else None))
            return _real(*a, **k)
        monkeypatch.setattr(ops, fn, counted)
    for fn in ('conv3x3_s2', 'conv3x3_grouped', 'conv7x7_s2', 'subsample2'):
        monkeypatch.setattr(ops, fn, lambda *a, _fn=fn, **k: pytest.fail(f'{_fn} ran'))
    with torch.no_grad():
        m(img)
    # 4 (stem) + 3 (layer1's stage block) + 3 * 4 (the stride-2 stage blocks) + 29 * 5 (normal blocks) = 164 for depth 101
    blocks = (3, 4, 23, 3)
    assert len(calls) == 4 + 3 + 3 * 4 + (sum(blocks) - 4) * 5 == 164
    slices = [(s, G) for fn, s, G in calls if fn == 'conv3x3_slices']
    assert slices.count((1, 3)) == 1 and slices.count((2, 3)) == 3 and slices.count((1, 1)) == 29 * 3 and len(slices) == 4 + 29 * 3
    names = [fn for fn, _, _ in calls]
    assert names[:4] == ['conv3x3_s2_c3', 'conv3x3_dil', 'conv3x3_dil', 'maxpool3x3_s2'] and names.count('conv3x3_dil') == 2
    assert names.count('avgpool2x2_ceil') == 3 and names.count('conv2d') == 2 * sum(blocks)


def test_chain_from_the_image_to_results(golden_dir):
    """``build_detector`` on the reference's whole r2_101 Mask R-CNN config, seeded weights, a 64 x 96 image: results of
    the right shapes, equal bit for bit to the parts composed by hand."""
    import backbone_inputs as bi
    import c4_inputs as ci
    import fpn_inputs as fi
    import res2net_inputs as xi
    import rpn_inputs as ri
    from dynamask_amd import backbones, build_detector
    with open(os.path.join(golden_dir, xi.CONFIGS)) as f:
        cfg = json.load(f)['mask_rcnn_r2_101']
    cfg['test_cfg']['rpn'].update(nms_post=24)
    det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert type(det.backbone) is backbones.Res2Net
    own = det.state_dict()
    state = {}
    for part, fn, seed in (('backbone', bi.head_state, bi.WEIGHT_SEED), ('neck', fi.head_state, fi.WEIGHT_SEED),
                           ('rpn_head', ri.head_state, 27), ('roi_head', ci.head_state, 27)):
        shapes = {k[len(part) + 1:]: v.shape for k, v in own.items() if k.startswith(part + '.')}
        state.update({f'{part}.{k}': v for k, v in fn(shapes, seed).items()})
    det.load_state_dict(state, strict=False)
    det = det.cuda().eval()
    H, W = 64, 96
    img = bi.inputs(1, H, W, seed=6496).cuda()
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False, flip_direction=None)]
    with torch.no_grad():
        stages = det.backbone(img)
        assert [tuple(s.shape) for s in stages] == [(1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
        assert all(bool(torch.isfinite(s).all()) and float(s.std()) > 0 for s in stages)
        bbox_results, segm_results = det.simple_test(img, metas)
        # by hand: the backbone, the neck, the RPN, the RoI head
        feats = det.neck(det.backbone(img))
        proposals = det.rpn_head.simple_test_rpn(feats, metas)
        bbox_hand, segm_hand = det.roi_head.simple_test(feats, proposals, metas, rescale=False)
    assert len(bbox_results) == 80 and len(segm_results) == 80
    for b, s, b2, s2 in zip(bbox_results, segm_results, bbox_hand, segm_hand):
        assert b.ndim == 2 and b.shape[1] == 5 and np.isfinite(b).all() and len(s) == len(b)
        assert all(tuple(np.asarray(mask).shape) == (H, W) for mask in s)
        assert b.tobytes() == b2.tobytes() and len(s) == len(s2)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(s, s2))
