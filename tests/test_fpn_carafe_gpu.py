"""FPN_CARAFE on the device: the whole-map CARAFE kernel (dm_carafe_map_fwd, csrc/carafe_map.hip) against
oracle.ref_ops.carafe_reassemble on the CPU in float32 and float64 at every output size, with and without the lateral
added, in place, at every channel split; what a NaN or an Inf reaches; the argument checks; ``necks.FPN_CARAFE`` against
the reference's own module (tests/golden/g32_fpn_carafe*.npz) and, step by step, against fpn_carafe_inputs.restate; the
launch count, host waits, batch independence; and the chain through the detector.

The kernel's tile is 8 x 32 INPUT pixels (MAP_TH x MAP_TW), one per thread, 8 channels per LDS chunk.  Of MAPS,
(1, 8, 1, 1), (1, 8, 2, 3) and (2, 16, 5, 7) sit inside one tile; (1, 8, 8, 32) fills one exactly; (1, 8, 9, 33) is one
pixel past both edges (2 x 2 tiles, three of them almost empty); (2, 64, 13, 21) crosses the row edge (2 x 1 tiles);
(1, 256, 3, 70) crosses the column edge twice (1 x 3 tiles) and has 32 chunks per group; (3, 24, 37, 53) crosses both
(5 x 2 tiles) with a ragged last chunk (6 quads, 3 at group 2)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

MAPS = [(1, 8, 1, 1), (1, 8, 2, 3), (2, 16, 5, 7), (2, 64, 13, 21), (1, 256, 3, 70), (3, 24, 37, 53), (1, 8, 8, 32), (1, 8, 9, 33)]
GUARD = 4096          # floats of NaN on either side of ``out``


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(NB, C, H, W, K, group, seed=0):
    s = NB * 1000003 + C * 10007 + H * 101 + W * 7 + K + group + seed
    x = torch.randn(NB, C, H, W, generator=_g(s))
    enc = torch.randn(NB, group * K * K * 4, H, W, generator=_g(s + 1)) * 1.5
    addend = torch.randn(NB, C, 2 * H, 2 * W, generator=_g(s + 2))
    return x, enc, addend


def _reference(x, enc, K, group):
    """carafe(x, softmax_taps(pixel_shuffle(enc))) at the full 2H x 2W on the CPU, in the dtype of ``x``."""
    from oracle import ref_ops
    mask = F.pixel_shuffle(enc, 2)
    n, mc, h, w = mask.shape
    mask = F.softmax(mask.view(n, group, K * K, h, w), dim=2).view(n, mc, h, w).contiguous()
    return ref_ops.carafe_reassemble(x, mask, K, group, 2)


def _guarded(shape, fill=float('nan')):
    """(out, whole): ``out`` of ``shape`` inside a NaN-filled buffer with GUARD floats on either side."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, device='cuda')
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


def _cases():
    out = []
    for m in MAPS:
        for K in (5, 3):
            for group in (1, 2):
                if (m[1] // group) % 4 == 0 and m[1] % group == 0:
                    out.append((m, K, group))
    return out


@pytest.mark.parametrize('m,K,group', _cases(), ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_against_float64(m, K, group):
    from dynamask_amd import ops
    NB, C, H, W = m
    x, enc, addend = _inputs(NB, C, H, W, K, group)
    up32, up64 = _reference(x, enc, K, group), _reference(x.double(), enc.double(), K, group)
    xd, ed = x.cuda(), enc.cuda()
    for OH in (2 * H - 1, 2 * H):
        for OW in (2 * W - 1, 2 * W):
            a = addend[:, :, :OH, :OW].contiguous()
            ad = a.cuda()
            for mode in ('plain', 'addend', 'inplace'):
                name = f'{m} K{K} g{group} -> {OH} x {OW} {mode}'
                r32 = up32[..., :OH, :OW] + (a if mode != 'plain' else 0)
                r64 = up64[..., :OH, :OW] + (a.double() if mode != 'plain' else 0)
                runs = []
                for _ in range(2):
                    if mode == 'inplace':        # out IS the addend: it starts from the lateral's values, inside NaN guards
                        out, whole = _guarded((NB, C, OH, OW))
                        out.copy_(ad)
                        got = ops.carafe_map(xd, ed, K, group, addend=out, out=out)
                    else:
                        out, whole = _guarded((NB, C, OH, OW))             # the NaN sentinel
                        got = ops.carafe_map(xd, ed, K, group, addend=ad if mode == 'addend' else None, out=out, out_size=(OH, OW))
                    assert got is out and bool(torch.isfinite(out).all()), f'{name}: an output was not written'
                    assert _guards_intact(whole), f'{name}: a write outside out'
                    runs.append(out.clone())
                assert torch.equal(_bits(runs[0]), _bits(runs[1])), f'{name}: two runs differ'
                err, ref_err, scale = assert_close_via_f64(runs[0], r32, r64, name)
                print(f'carafe_map {name}: |product - f64| {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
            assert torch.equal(ad.cpu(), a), 'the out-of-place addend was written'
    assert torch.equal(xd.cpu(), x) and torch.equal(ed.cpu(), enc), 'x or enc was written'
    # a new tensor of the default size
    got = ops.carafe_map(xd, ed, K, group)
    assert tuple(got.shape) == (NB, C, 2 * H, 2 * W)
    assert_close_via_f64(got, up32, up64, f'{m} K{K} g{group} default')


@pytest.mark.parametrize('m', [(2, 64, 13, 21), (1, 256, 3, 70)], ids=str)
@pytest.mark.parametrize('K,group', [(5, 1), (3, 2)])
def test_bits_do_not_depend_on_the_channel_split(m, K, group):
    from dynamask_amd import ops
    NB, C, H, W = m
    x, enc, addend = _inputs(NB, C, H, W, K, group, seed=5)
    xd, ed = x.cuda(), enc.cuda()
    ad = addend[:, :, :2 * H - 1, :].contiguous().cuda()
    quads = C // group // 4
    outs = [ops.carafe_map(xd, ed, K, group, addend=ad, chan_split=s) for s in (1, quads, 0, 3, quads - 1)]
    for o in outs[1:]:
        assert torch.equal(_bits(o), _bits(outs[0]))
    assert bool(torch.isfinite(outs[0]).all())
    with pytest.raises(RuntimeError, match='dm_carafe_map_fwd'):
        ops.carafe_map(xd, ed, K, group, addend=ad, chan_split=quads + 1)


@pytest.mark.parametrize('m,K,group', [((2, 16, 5, 7), 5, 1), ((1, 8, 9, 33), 3, 2), ((3, 24, 37, 53), 5, 2)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_cropped_add_is_the_composed_call(m, K, group):
    from dynamask_amd import ops
    NB, C, H, W = m
    x, enc, addend = _inputs(NB, C, H, W, K, group, seed=9)
    xd, ed = x.cuda(), enc.cuda()
    full = ops.carafe_map(xd, ed, K, group)
    for OH in (2 * H - 1, 2 * H):
        for OW in (2 * W - 1, 2 * W):
            ad = addend[:, :, :OH, :OW].contiguous().cuda()
            fused = ops.carafe_map(xd, ed, K, group, addend=ad)
            assert torch.equal(_bits(fused), _bits(ad + full[:, :, :OH, :OW]))
            assert torch.equal(_bits(ops.carafe_map(xd, ed, K, group, out_size=(OH, OW))), _bits(full[:, :, :OH, :OW]))


def test_a_four_byte_aligned_out_takes_the_scalar_stores():
    """``out`` and ``addend`` at an odd float offset of their buffers: the pair stores need 8-byte alignment, the launcher
    falls back to scalar stores and the bits stay."""
    from dynamask_amd import ops
    NB, C, H, W, K, group = 2, 16, 5, 7, 5, 1
    x, enc, addend = _inputs(NB, C, H, W, K, group, seed=21)
    xd, ed, ad = x.cuda(), enc.cuda(), addend.cuda()
    want = ops.carafe_map(xd, ed, K, group, addend=ad)
    n = want.numel()
    for off_out, off_add in ((1, 0), (0, 1), (1, 1)):
        whole = torch.full((n + 2 * GUARD,), float('nan'), device='cuda')
        out = whole[GUARD + off_out:GUARD + off_out + n].view(want.shape)
        abuf = torch.empty(n + 1, device='cuda')
        a = abuf[off_add:off_add + n].view(want.shape)
        a.copy_(ad)
        assert out.data_ptr() % 8 == 4 * off_out and a.data_ptr() % 8 == 4 * off_add
        ops.carafe_map(xd, ed, K, group, addend=a, out=out)
        assert torch.equal(_bits(out), _bits(want))
        assert bool(torch.isnan(whole[:GUARD + off_out]).all()) and bool(torch.isnan(whole[GUARD + off_out + n:]).all())


@pytest.mark.parametrize('K', [5, 3])
@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_a_non_finite_input_reaches_its_windows_only(K, value):
    from dynamask_amd import ops
    NB, C, H, W, group = 2, 8, 9, 33, 1
    R = K // 2
    x, enc, _ = _inputs(NB, C, H, W, K, group, seed=13)
    ed = enc.cuda()
    clean = ops.carafe_map(x.cuda(), ed, K, group)
    assert bool(torch.isfinite(clean).all())
    for (n, c, py, px) in ((1, 5, 4, 17), (0, 0, 0, 0), (1, 7, H - 1, W - 1), (0, 3, 7, 31), (0, 3, 8, 32)):
        bad = x.clone()
        bad[n, c, py, px] = value
        got = ops.carafe_map(bad.cuda(), ed, K, group).cpu()
        want = torch.zeros(NB, C, 2 * H, 2 * W, dtype=torch.bool)
        want[n, c, max(0, 2 * (py - R)):2 * (py + R) + 2, max(0, 2 * (px - R)):2 * (px + R) + 2] = True
        ref = _reference(bad, enc, K, group)
        assert torch.equal(~torch.isfinite(ref), want), 'the reference does not reach the windows that hold the pixel'
        assert torch.equal(~torch.isfinite(got), want), f'{value} at {(n, c, py, px)}: {int((~torch.isfinite(got)).sum())} non-finite outputs, {int(want.sum())} expected'
        assert torch.equal(_bits(got)[~want], _bits(clean.cpu())[~want]), 'a clean output changed'


def test_a_nan_in_enc_reaches_one_output_pixel_of_its_group():
    from dynamask_amd import ops
    NB, C, H, W, K, group = 1, 16, 9, 33, 5, 2
    x, enc, addend = _inputs(NB, C, H, W, K, group, seed=17)
    xd = x.cuda()
    clean = ops.carafe_map(xd, enc.cuda(), K, group).cpu()
    for (g, kk, sub, y, xx) in ((1, 7, 2, 4, 17), (0, 0, 0, 0, 0), (1, 24, 3, H - 1, W - 1)):
        bad = enc.clone()
        bad[0, (g * K * K + kk) * 4 + sub, y, xx] = float('nan')
        got = ops.carafe_map(xd, bad.cuda(), K, group).cpu()
        want = torch.zeros(NB, C, 2 * H, 2 * W, dtype=torch.bool)
        want[0, g * 8:(g + 1) * 8, 2 * y + sub // 2, 2 * xx + sub % 2] = True
        assert torch.equal(torch.isnan(_reference(x, bad, K, group)), want)
        assert torch.equal(torch.isnan(got), want)
        assert torch.equal(_bits(got)[~want], _bits(clean)[~want])


def test_argument_checks():
    from dynamask_amd import _lib, ops
    L = _lib.lib()
    x, enc, addend = _inputs(1, 8, 2, 3, 5, 1)
    xd, ed, ad = x.cuda(), enc.cuda(), addend.cuda()
    out = torch.empty(1, 8, 4, 6, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731

    def call(x=xd, enc=ed, NB=1, C=8, H=2, W=3, K=5, group=1, addend=ad, OH=4, OW=6, split=0, out=out):
        return L.dm_carafe_map_fwd(p(x), p(enc), NB, C, H, W, K, group, p(addend), OH, OW, split, p(out), None)
    assert call() == 0 and call(addend=None) == 0
    assert call(x=None) == -1 and call(enc=None) == -1 and call(out=None) == -1
    assert call(NB=-1) == -1 and call(C=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(group=0) == -1
    assert call(split=-1) == -1 and call(split=3) == -1 and call(split=2) == 0
    # every refusal of dm_carafe_map_supported
    assert call(K=4) == -3 and call(K=7) == -3 and call(K=1) == -3
    assert call(group=3) == -3                               # C % group
    assert call(group=4) == -3                               # 2 channels per group
    assert call(OH=2) == -3 and call(OH=5) == -3 and call(OW=4) == -3 and call(OW=7) == -3
    assert call(C=1 << 20, H=32, W=64, OH=64, OW=128) == -3  # 2^31 elements of x
    assert call(NB=0) == 0 and call(NB=0, x=None, enc=None, out=None) == 0
    torch.cuda.synchronize()
    # the wrapper
    with pytest.raises(RuntimeError, match='dm_carafe_map_fwd'):
        ops.carafe_map(xd, torch.zeros(1, 64, 2, 3, device='cuda'), up_kernel=4)
    with pytest.raises(RuntimeError, match='dm_carafe_map_fwd'):
        ops.carafe_map(xd, ed, out_size=(2, 6))
    with pytest.raises(ValueError, match='enc'):
        ops.carafe_map(xd, ed, up_kernel=3)
    with pytest.raises(ValueError, match='addend'):
        ops.carafe_map(xd, ed, addend=ad, out_size=(3, 6))
    with pytest.raises(ValueError, match='out'):
        ops.carafe_map(xd, ed, out=torch.empty(1, 8, 3, 6, device='cuda'), out_size=(4, 6))
    with pytest.raises(ValueError, match='contiguous'):
        ops.carafe_map(xd, ed, addend=addend.cuda()[:, :, :, :5])
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.carafe_map(x, ed)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.carafe_map(xd, ed, addend=addend)
    with pytest.raises(TypeError):
        ops.carafe_map(xd.double(), ed)
    empty = ops.carafe_map(xd[:0], ed[:0], out_size=(3, 5))
    assert tuple(empty.shape) == (0, 8, 3, 5)
    assert tuple(ops.carafe_map(xd[:0], ed[:0], addend=ad[:0]).shape) == (0, 8, 4, 6)


# ------------------------------------------------------------------------------------------------ the neck
@pytest.fixture(scope='module')
def neck(golden_dir):
    """(FPN_CARAFE on the device with the fixture's weights, the stages on the device, the config, the state, the inputs module)."""
    import fpn_carafe_inputs as ci
    from dynamask_amd import necks, registry  # noqa: F401
    with open(os.path.join(golden_dir, ci.CONFIGS)) as f:
        cfg = json.load(f)[ci.NECK_ENTRY]
    m = registry.build_neck(dict(cfg['model']['neck']))
    state = ci.head_state({k: v.shape for k, v in m.state_dict().items()}, ci.WEIGHT_SEED)
    m.load_state_dict(state, strict=True)
    m = m.cuda().eval()
    xs = [x.cuda() for x in ci.inputs(m.in_channels, ci.BATCH, seed=ci.FEAT_SEED)]
    return m, xs, cfg['model']['neck'], state, ci


def test_forward_against_the_reference(neck, golden_dir):
    from dynamask_amd import conv_precision, necks
    m, xs, _, _, ci = neck
    z = {}
    for name in sorted(set(ci.FILES)):
        z.update(np.load(os.path.join(golden_dir, name)))
    assert necks.FPN_CARAFE_FUSED[0]
    before = [x.clone() for x in xs]
    with torch.no_grad():
        outs = m(xs)
        again = m(xs)
        with conv_precision('bf16x3'):
            outs3 = m(xs)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(xs, before)), 'forward wrote into its inputs'
    assert isinstance(outs, tuple) and len(outs) == m.num_outs == 5
    for l, (got, second, other) in enumerate(zip(outs, again, outs3)):
        ref32 = z[f'out{l}']
        assert tuple(got.shape) == ref32.shape, f'level {l}'
        err, ref_err, scale = assert_close_via_f64(got, ref32, ci.unpack_f64(ref32, z[f'out{l}_err16']), f'level {l}')
        print(f'FPN_CARAFE level {l}: |product - f64| {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
        assert torch.equal(_bits(got), _bits(second)), f'level {l}: two calls differ'
        assert torch.equal(_bits(got), _bits(other)), f'level {l}: the bf16x3 mode changed the neck'


def test_every_top_down_step_on_the_restatements_input(neck):
    """Each merge on the restatement's own input to it: an error shows at the level that makes it."""
    from dynamask_amd import ops
    m, xs, cfg, state, ci = neck
    cpu = [x.cpu() for x in xs]
    with torch.no_grad():
        _, steps32 = ci.restate(cfg, state, cpu, every_level=True)
        _, steps64 = ci.restate(cfg, state, [x.double() for x in cpu], every_level=True)
        assert [s['level'] for s in steps32] == [4, 3, 2, 1]
        for s32, s64 in zip(steps32, steps64):
            i = s32['level']
            src, lat = s32['src'].cuda(), s32['lat'].cuda()
            enc = m.upsample_modules[i - 1].encode(src)
            assert_close_via_f64(enc, s32['enc'], s64['enc'], f'step {i}: the encoder')
            got = ops.carafe_map(src, enc, m.up_kernel, m.up_group, addend=lat)
            assert tuple(got.shape) == tuple(s32['merged'].shape)
            err, ref_err, scale = assert_close_via_f64(got, s32['merged'], s64['merged'], f'step {i}: lateral {i - 1} merged')
            print(f'step {i}: |product - f64| {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
            # on the restatement's own encoder output the reassembly alone
            alone = ops.carafe_map(src, s32['enc'].cuda(), m.up_kernel, m.up_group, addend=lat)
            assert_close_via_f64(alone, s32['merged'], s64['merged'], f'step {i}: the reassembly alone')


def test_launches_host_waits_batch_independence_and_the_composed_path(neck, monkeypatch):
    import bench
    from dynamask_amd import necks, ops
    m, xs, _, _, ci = neck
    with torch.no_grad():
        fused = m(xs)
        assert bench.count_host_syncs(lambda: m(xs)) == 0
        # B = 1 against image 0 of B = 2
        two = [x.cuda() for x in ci.inputs(m.in_channels, 2, seed=ci.FEAT_SEED)]
        assert all(torch.equal(a[0], b[0]) for a, b in zip(two, xs))
        both = m(two)
        for l, (a, b) in enumerate(zip(fused, both)):
            assert tuple(b.shape) == (2,) + tuple(a.shape[1:])
            assert torch.equal(_bits(a[0]), _bits(b[0])), f'level {l}: an image\'s bits depend on the batch'
        # the composed merge gives the same bits
        monkeypatch.setattr(necks, 'FPN_CARAFE_FUSED', [False])
        composed = m(xs)
        monkeypatch.setattr(necks, 'FPN_CARAFE_FUSED', [True])
        for l, (a, b) in enumerate(zip(fused, composed)):
            assert torch.equal(_bits(a), _bits(b)), f'level {l}: {int((a != b).sum())} values differ'
    calls = []
    for fn in ('conv2d', 'conv3x3_s2', 'conv3x3_dil', 'carafe_map'):
        def counted(*a, _real=getattr(ops, fn), _fn=fn, **k):
            calls.append((_fn, 'addend' in k and k['addend'] is not None and k.get('out') is k['addend']))
            return _real(*a, **k)
        monkeypatch.setattr(ops, fn, counted)
    for fn in ('carafe', 'conv2d_up_add', 'subsample2'):
        monkeypatch.setattr(ops, fn, lambda *a, _fn=fn, **k: pytest.fail(f'{_fn} ran'))
    with torch.no_grad():
        m(xs)
    names = [fn for fn, _ in calls]
    # 4 laterals + the extra level + 4 x (compressor, encoder, carafe_map) + 5 level convolutions
    assert len(calls) == 22 and names.count('carafe_map') == 4 and names.count('conv3x3_s2') == 1 and names.count('conv2d') == 17
    assert all(inplace for fn, inplace in calls if fn == 'carafe_map')
    assert names[:5] == ['conv2d'] * 4 + ['conv3x3_s2'] and names[5:17] == ['conv2d', 'conv2d', 'carafe_map'] * 4


def test_forward_on_a_wide_map(monkeypatch):
    """The encoder and the level convolution leave ops.conv2d for the any-width 3x3 kernel above CONV2D_3X3_MAX_WIDTH."""
    import fpn_carafe_inputs as ci
    from dynamask_amd import necks, ops
    cfg = dict(in_channels=[8, 16, 16], out_channels=8, num_outs=3,
               upsample_cfg=dict(type='carafe', up_kernel=3, up_group=2, encoder_kernel=3, encoder_dilation=1, compressed_channels=8))
    m = necks.FPN_CARAFE(**cfg)
    state = ci.head_state({k: v.shape for k, v in m.state_dict().items()}, 130)
    m.load_state_dict(state, strict=True)
    m = m.cuda().eval()
    xs = ci.inputs([8, 16, 16], 2, seed=130, sizes=((4, 259), (2, 130), (1, 65)))
    routes = []
    real = ops.conv3x3_dil
    monkeypatch.setattr(ops, 'conv3x3_dil', lambda x, *a, **k: (routes.append(tuple(x.shape)), real(x, *a, **k))[1])
    with torch.no_grad():
        outs = m([x.cuda() for x in xs])
        ref32 = ci.restate(cfg, state, xs)
        ref64 = ci.restate(cfg, state, [x.double() for x in xs])
    assert routes == [(2, 8, 2, 130), (2, 8, 4, 259), (2, 8, 2, 130)]      # the encoder of step 1, then two level convolutions
    assert [tuple(o.shape) for o in outs] == [(2, 8, 4, 259), (2, 8, 2, 130), (2, 8, 1, 65)]
    for l in range(3):
        assert_close_via_f64(outs[l], ref32[l], ref64[l], f'wide map, level {l}')
    # a lateral the level above does not upsample into
    odd = ci.inputs([8, 16, 16], 1, seed=131, sizes=((5, 20), (2, 10), (1, 5)))
    with torch.no_grad(), pytest.raises(NotImplementedError, match='does not upsample'):
        m([x.cuda() for x in odd])


def test_chain_from_the_image_to_results(golden_dir):
    """``build_detector`` on the reference's whole Mask R-CNN CARAFE config, seeded weights, a 64 x 96 image: results of
    the right shapes, equal bit for bit to the parts composed by hand."""
    import backbone_inputs as bi
    import c4_inputs as c4
    import fpn_carafe_inputs as ci
    import rpn_inputs as ri
    from dynamask_amd import backbones, build_detector, necks
    with open(os.path.join(golden_dir, ci.CONFIGS)) as f:
        cfg = json.load(f)['mask_rcnn_carafe']
    cfg['test_cfg']['rpn'].update(nms_post=24)
    det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert type(det.backbone) is backbones.ResNet and type(det.neck) is necks.FPN_CARAFE
    assert det.roi_head.mask_head.upsample_method == 'carafe'
    own = det.state_dict()
    state = {}
    for part, fn, seed in (('backbone', bi.head_state, bi.WEIGHT_SEED), ('neck', ci.head_state, ci.WEIGHT_SEED),
                           ('rpn_head', ri.head_state, 27), ('roi_head', c4.head_state, 27)):
        shapes = {k[len(part) + 1:]: v.shape for k, v in own.items() if k.startswith(part + '.')}
        state.update({f'{part}.{k}': v for k, v in fn(shapes, seed).items()})
    det.load_state_dict(state, strict=False)
    det = det.cuda().eval()
    H, W = 64, 96
    img = bi.inputs(1, H, W, seed=6496).cuda()
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False, flip_direction=None)]
    with torch.no_grad():
        bbox_results, segm_results = det.simple_test(img, metas)
        # by hand
        stages = det.backbone(img)
        assert [tuple(s.shape) for s in stages] == [(1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
        feats = det.neck(stages)
        assert [tuple(f.shape) for f in feats] == [(1, 256, 16, 24), (1, 256, 8, 12), (1, 256, 4, 6), (1, 256, 2, 3), (1, 256, 1, 2)]
        assert all(bool(torch.isfinite(f).all()) and float(f.std()) > 0 for f in feats)
        proposals = det.rpn_head.simple_test_rpn(feats, metas)
        assert len(proposals) == 1 and 0 < len(proposals[0]) <= 24
        bbox_hand, segm_hand = det.roi_head.simple_test(feats, proposals, metas, rescale=False)
    assert len(bbox_results) == 80 and len(segm_results) == 80
    for b, s, b2, s2 in zip(bbox_results, segm_results, bbox_hand, segm_hand):
        assert b.ndim == 2 and b.shape[1] == 5 and np.isfinite(b).all() and len(s) == len(b)
        assert all(tuple(np.asarray(mask).shape) == (H, W) for mask in s)
        assert b.tobytes() == b2.tobytes() and len(s) == len(s2)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(s, s2))
