"""The fused inference launches at every shape their support checks accept, and just past them.

Each fused launch of round 6 claims the bits of the launch sequence it replaces; the bit tests of test_ops_gpu.py hold
that claim at the DynaMask stage shapes only (256 / 128 / 64 channels, 14 / 28 / 56 pixels, 80 classes).  Inside the
kernels the tile layout is chosen at compile time from the shape, so the places where the host and the kernel could
disagree are the other shapes the host accepts.  Every case here checks
  (a) the fused launch against the unfused ``ops`` sequence, bit for bit (``torch.equal``),
  (b) the same outputs against a float64 CPU reference (``tolerances.assert_close_via_f64``, with the same computation in
      float32 on the CPU as the fp32 reference),
  (c) that a canary written around the outputs (channels past the ones the launch owns, rows past its last RoI) survives,
and, for the shapes a support check refuses, that the launch raises and leaves its outputs as they were.  Thresholds
that depend on the device (the few-RoI layout of the DCN) are found by asking the support predicate, not hard-coded."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model, ref_ops
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

CANARY = 7.0


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t):
    return t.cuda().contiguous()


def _canary(*shape):
    return torch.full(shape, CANARY, device='cuda')


def _untouched(t, what):
    assert bool((t == CANARY).all()), f'{what}: the canary was overwritten'


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


# ----------------------------------------------------------------------------------------------- DCN + chained 1x1
def _tout_ok(ops, NB, C, H, W, m2):
    return ops.deform_conv_tout_supported(torch.empty((NB, C, H, W), device='meta'), C, m2)


def _first_tout_nb(ops, C, H, W, m2):
    """Fewest RoIs the fused DCN + 1x1 takes at this map (below: the few-RoI layout, which cannot chain the 1x1)."""
    for nb in range(1, 1025):
        if _tout_ok(ops, nb, C, H, W, m2):
            assert _tout_ok(ops, nb + 7, C, H, W, m2), 'the predicate is not monotone in the RoI count'
            return nb
    return None


def _tout_inputs(NB, C, H, W, seed):
    gen = _g(seed)
    x = torch.randn(NB, C, H, W, generator=gen)
    off = torch.randn(NB, 36, H, W, generator=gen) * 1.5
    off[0, :, :4, :4] = 9.0                           # far samples: the band kernel's slow pass
    off[-1, ::2, H // 2] = 25.0                       # a row of pixels looking 25 rows down / up, clamped at the borders
    off[-1, ::2, H // 2 + 1] = -25.0
    off[-1, 18:, :, W // 2] = 0.0                     # group 1 of the last image: plain taps in one column
    w = torch.randn(C, C, 3, 3, generator=gen) / (9 * C) ** 0.5
    return x, off, w


def _tout_weights(m2, C, seed):
    gen = _g(seed)
    # (a small positive bias: most outputs pass the ReLU, so the tensor's scale is that of the sums being compared)
    return torch.randn(m2, C, 1, 1, generator=gen) / C ** 0.5, torch.rand(m2, generator=gen) * 0.5 + 0.25


# (C, H, W): maps with H >= 16 and W % 4 == 0 the band kernel takes, square and not, of 560 / 512 / 784 / 3136 pixels (a
# ragged last 128-pixel tile in all but 512); the M2 the 1x1 build of the channel count has room for (C = 64: one 32-cout
# tile, C = 128: two) and the ones past it
TOUT_SHAPES = [
    (128, 28, 28, (1, 8, 31, 32, 33, 62, 64), (65, 96)),
    (128, 16, 32, (1, 32, 33, 64), (65,)),
    (128, 20, 28, (8, 40), ()),
    (64, 20, 28, (1, 8, 31, 32), (33, 62, 64, 65)),
    (64, 16, 32, (8, 32), (33,)),
    (64, 28, 28, (1, 31), (62,)),
    (64, 56, 56, (8, 30, 32), (33,)),
]


@pytest.mark.parametrize('C,H,W,m2s,refused', TOUT_SHAPES)
def test_dcn_tout_sweep_has_the_bits_of_the_two_launches_and_matches_f64(ops, C, H, W, m2s, refused):
    NB = _first_tout_nb(ops, C, H, W, m2s[0])
    assert NB is not None, (C, H, W)
    for m2 in m2s:
        assert _first_tout_nb(ops, C, H, W, m2) == NB, m2          # the RoI threshold does not depend on M2
    x32, off32, w32 = _tout_inputs(NB, C, H, W, 1000 + C + H + W)
    x, off, w = _dev(x32), _dev(off32), _dev(w32)
    wp = ops.pack_conv_weight(w)
    d_ref = ops.deform_conv(x, off, wp, C, 2, relu=True)
    # float64 / float32 CPU oracle of relu(DCN) on the first and the last RoI (the far and the +-25-row offsets)
    rows = [0, NB - 1]
    d64 = F.relu(ref_ops.deform_conv2d(x32[rows].double(), off32[rows].double(), w32.double(), 1, 1, 1, 2))
    d32 = F.relu(ref_ops.deform_conv2d(x32[rows], off32[rows], w32, 1, 1, 1, 2))
    assert_close_via_f64(d_ref[rows], d32, d64, f'relu(DCN) C={C} {H}x{W}')
    for m2 in m2s:
        w2_32, b2_32 = _tout_weights(m2, C, 2000 + m2)
        w2, b2 = _dev(w2_32), _dev(b2_32)
        w2p, w2t = ops.pack_conv_weight(w2), ops.pack_tout_weight(w2)
        assert tuple(w2t.shape) == (C, (m2 + 31) // 32 * 32)
        ct = m2 + 3                                               # out2 wider than M2: three canary channels behind it
        t_ref = _canary(NB, ct, H, W)
        ops.conv2d(d_ref, w2p, b2, m2, 1, relu=True, out=t_ref, out_ch_offset=0)
        for keep in (False, True):
            t = _canary(NB, ct, H, W)
            d = ops.deform_conv_tout(x, off, wp, C, 2, w2t, b2, m2, t, keep_dcn=keep)
            assert torch.equal(t, t_ref), (C, H, W, m2, keep)
            _untouched(t[:, m2:], f'out2 channels past M2 = {m2}')
            assert (d is None) if not keep else torch.equal(d, d_ref)
        buf = _canary(NB + 1, C, H, W)                             # relu(DCN) into a caller's buffer: one canary row behind it
        t = _canary(NB, ct, H, W)
        assert ops.deform_conv_tout(x, off, wp, C, 2, w2t, b2, m2, t, dcn_out=buf[:NB]) is not None
        assert torch.equal(buf[:NB], d_ref) and torch.equal(t, t_ref), (C, H, W, m2)
        _untouched(buf[NB], 'the row behind dcn_out')
        t64 = F.relu(F.conv2d(d64, w2_32.double(), b2_32.double()))
        t32 = F.relu(F.conv2d(d32, w2_32, b2_32))
        assert_close_via_f64(t[rows, :m2], t32, t64, f'DCN + 1x1 C={C} {H}x{W} M2={m2}')
    for m2 in refused:
        assert not _tout_ok(ops, NB, C, H, W, m2), m2
        _assert_tout_refused(ops, x, off, wp, C, m2)
    if NB > 1:                                                    # one RoI fewer: the few-RoI layout, refused
        assert not _tout_ok(ops, NB - 1, C, H, W, m2s[0])
        _assert_tout_refused(ops, x[:NB - 1].contiguous(), off[:NB - 1].contiguous(), wp, C, m2s[0])


def _assert_tout_refused(ops, x, off, wp, C, m2):
    NB, _, H, W = x.shape
    w2 = _dev(torch.randn(m2, C, 1, 1, generator=_g(3000 + m2)))
    t = _canary(NB, m2 + 1, H, W)
    buf = _canary(NB, C, H, W)
    with pytest.raises(RuntimeError, match='not supported'):
        ops.deform_conv_tout(x, off, wp, C, 2, ops.pack_tout_weight(w2), _dev(torch.zeros(m2)), m2, t, dcn_out=buf)
    torch.cuda.synchronize()
    _untouched(t, f'out2 of a refused shape C={C} {H}x{W} M2={m2}')
    _untouched(buf, f'dcn_out of a refused shape C={C} {H}x{W} M2={m2}')


# maps the band kernel does not take, or takes in a layout that cannot chain the 1x1: W > 32 at 128 channels (two waves
# share a pixel column), W % 4 != 0, H < 16, W < 28 (a 128-pixel tile spans too many rows for the +-5-row band), 256 channels
@pytest.mark.parametrize('C,H,W', [(128, 28, 40), (128, 56, 56), (64, 30, 30), (64, 14, 28), (64, 24, 24), (64, 32, 20),
                                   (256, 28, 28)])
def test_dcn_tout_refuses_the_maps_it_has_no_build_for(ops, C, H, W):
    NB = 64
    m2 = C // 2 - 2
    assert not _tout_ok(ops, NB, C, H, W, m2)
    assert _first_tout_nb(ops, C, H, W, m2) is None
    gen = _g(4000 + C + H + W)
    x = _dev(torch.randn(NB, C, H, W, generator=gen))
    off = _dev(torch.randn(NB, 36, H, W, generator=gen))
    wp = ops.pack_conv_weight(_dev(torch.randn(C, C, 3, 3, generator=gen) / (9 * C) ** 0.5))
    _assert_tout_refused(ops, x, off, wp, C, m2)


# ----------------------------------------------------------------------------------------------- stage head
def _logit_weights(nc, C, seed):
    gen = _g(seed)
    return (torch.randn(nc, C, generator=gen) / C ** 0.5, torch.randn(nc, generator=gen),
            torch.randn(nc, C, generator=gen) / C ** 0.5, torch.randn(nc, generator=gen))


def _labels(N, nc, seed):
    lab = torch.randint(0, nc, (N,), generator=_g(seed))
    lab[0] = 0
    lab[-1] = nc - 1
    return lab


def _class_logits_f64(x, wi, bi, wd, bd, labels):
    nc, C = wi.shape
    ar = torch.arange(x.shape[0])
    return (F.conv2d(x, wi.view(nc, C, 1, 1), bi)[ar, labels][:, None], F.conv2d(x, wd.view(nc, C, 1, 1), bd)[ar, labels][:, None])


# (N, C, Cs, S, nc): semantic channels that are not a multiple of the 16-channel chunk, the four point-sample sizes, the
# class counts of the reference configs; one RoI, and more RoIs than one 256-position block holds
STAGE_HEAD = [
    (1, 64, 24, 7, 80),
    (37, 37, 40, 7, 8),
    (5, 128, 24, 14, 1),
    (1, 30, 40, 20, 80),
    (11, 64, 16, 20, 8),
    (3, 96, 40, 28, 80),
    (9, 128, 24, 28, 1),
]


@pytest.mark.parametrize('N,C,Cs,S,nc', STAGE_HEAD)
def test_stage_head_sweep_has_the_bits_of_its_two_launches_and_matches_f64(ops, N, C, Cs, S, nc):
    gen = _g(5000 + N + C + Cs + S + nc)
    H, W, scale = 37, 53, 0.25
    sem32 = torch.randn(2, Cs, H, W, generator=gen)
    x32 = torch.randn(N, C, S, S, generator=gen)
    # RoIs of two images (sorted by image, as bbox2roi gives them) of the 212 x 148 image, some reaching past its borders
    nb0 = (N + 1) // 2
    xy = torch.rand(N, 2, generator=gen) * 120 - 10
    wh = torch.rand(N, 2, generator=gen) * 90 + 4
    rois32 = torch.cat([(torch.arange(N) >= nb0).float()[:, None], xy, xy + wh], 1)
    lab = _labels(N, nc, 5100 + N)
    wi32, bi32, wd32, bd32 = _logit_weights(nc, C, 5200 + C + nc)
    sem, x, rois, labels = _dev(sem32), _dev(x32), _dev(rois32), lab.cuda()
    wts = [_dev(t) for t in (wi32, bi32, wd32, bd32)]
    sig_a, sig_b = _canary(N, 6, S, S), _canary(N, 6, S, S)
    ps = ops.point_sample(sem, rois, S, scale)
    ip, dp = ops.class_logits(x, *wts, labels, sig_out=sig_a, sig_ch_offset=3)
    oi, od = _canary(N + 2, 1, S, S), _canary(N + 2, 1, S, S)       # two canary rows behind the N the launch owns
    ps2, ip2, dp2 = ops.stage_head(sem, rois, S, scale, x, *wts, labels, sig_out=sig_b, sig_ch_offset=3, out=(oi[:N], od[:N]))
    assert torch.equal(ps, ps2) and torch.equal(ip, ip2) and torch.equal(dp, dp2) and torch.equal(sig_a, sig_b)
    _untouched(oi[N:], 'rows behind inst')
    _untouched(od[N:], 'rows behind det')
    _untouched(sig_b[:, :3], 'sig_out channels before the offset')
    _untouched(sig_b[:, 5:], 'sig_out channels behind the two logits')
    p64 = ref_ops.simple_roi_align(sem32.double(), rois32.double(), S, scale)
    p32 = ref_ops.simple_roi_align(sem32, rois32, S, scale)
    assert_close_via_f64(ps2, p32, p64, f'point sample Cs={Cs} S={S}')
    r64 = _class_logits_f64(x32.double(), wi32.double(), bi32.double(), wd32.double(), bd32.double(), lab)
    r32 = _class_logits_f64(x32, wi32, bi32, wd32, bd32, lab)
    for got, a, b, name in ((ip2, r32[0], r64[0], 'inst'), (dp2, r32[1], r64[1], 'det')):
        assert_close_via_f64(got, a, b, f'{name} logits C={C} S={S} nc={nc}')
    assert_close_via_f64(sig_b[:, 3:5], torch.cat(r32, 1).sigmoid(), torch.cat(r64, 1).sigmoid(), 'sig_out')
    # refused: the two sigmoid channels do not fit behind the offset -- nothing is written
    sig_c = _canary(N, 6, S, S)
    oi_c, od_c = _canary(N, 1, S, S), _canary(N, 1, S, S)
    with pytest.raises(RuntimeError, match='invalid argument'):
        ops.stage_head(sem, rois, S, scale, x, *wts, labels, sig_out=sig_c, sig_ch_offset=5, out=(oi_c, od_c))
    torch.cuda.synchronize()
    for t, name in ((sig_c, 'sig_out'), (oi_c, 'inst'), (od_c, 'det')):
        _untouched(t, f'{name} of a refused stage head')


# ----------------------------------------------------------------------------------------------- class logits on the x2 upsample
# (N, C, H, W, nc): odd H, H = 2, W = 2, W = 2 mod 4 (an odd number of column pairs), channel counts whose last group of
# eight is partial (30, 62) or full (128)
UP2X = [
    (3, 30, 7, 6, 80),
    (2, 62, 2, 8, 1),
    (4, 128, 5, 2, 80),
    (1, 30, 9, 10, 1),
    (70, 62, 3, 14, 80),
    (2, 128, 14, 14, 1),
]


@pytest.mark.parametrize('N,C,H,W,nc', UP2X)
def test_class_logits_up2x_sweep_has_the_bits_of_its_two_launches_and_matches_f64(ops, N, C, H, W, nc):
    gen = _g(6000 + N + C + H + W + nc)
    x32 = torch.randn(N, C, H, W, generator=gen)
    lab = _labels(N, nc, 6100 + N)
    wi32, bi32, wd32, bd32 = _logit_weights(nc, C, 6200 + C + nc)
    x, labels = _dev(x32), lab.cuda()
    wts = [_dev(t) for t in (wi32, bi32, wd32, bd32)]
    assert ops.class_logits_up2x_supported(x)
    oi, od = _canary(N + 1, 1, 2 * H, 2 * W), _canary(N + 1, 1, 2 * H, 2 * W)
    gi, gd = ops.class_logits_up2x(x, *wts, labels, out=(oi[:N], od[:N]))
    _untouched(oi[N], 'the row behind inst')
    _untouched(od[N], 'the row behind det')
    ti, td = ops.class_logits(ops.upsample2x(x, align_corners=False, relu=True), *wts, labels)
    assert torch.equal(gi, ti) and torch.equal(gd, td)
    # the kernel applies the ReLU to the upsampled values (pointwise.hip: dm_up2x_interp, then fmaxf)
    up64 = F.relu(F.interpolate(x32.double(), scale_factor=2, mode='bilinear', align_corners=False))
    up32 = F.relu(F.interpolate(x32, scale_factor=2, mode='bilinear', align_corners=False))
    r64 = _class_logits_f64(up64, wi32.double(), bi32.double(), wd32.double(), bd32.double(), lab)
    r32 = _class_logits_f64(up32, wi32, bi32, wd32, bd32, lab)
    assert_close_via_f64(gi, r32[0], r64[0], f'up2x inst C={C} {H}x{W} nc={nc}')
    assert_close_via_f64(gd, r32[1], r64[1], f'up2x det C={C} {H}x{W} nc={nc}')


@pytest.mark.parametrize('H,W', [(6, 7), (2, 3), (1, 8), (1, 2)])
def test_class_logits_up2x_refuses_odd_widths_and_single_rows(ops, H, W):
    N, C, nc = 2, 30, 8
    x = _dev(torch.randn(N, C, H, W, generator=_g(6300 + H + W)))
    wts = [_dev(t) for t in _logit_weights(nc, C, 6301)]
    assert not ops.class_logits_up2x_supported(x)
    oi, od = _canary(N, 1, 2 * H, 2 * W), _canary(N, 1, 2 * H, 2 * W)
    with pytest.raises(RuntimeError, match='not supported'):
        ops.class_logits_up2x(x, *wts, torch.zeros(N, dtype=torch.int64).cuda(), out=(oi, od))
    torch.cuda.synchronize()
    _untouched(oi, 'inst of a refused shape')
    _untouched(od, 'det of a refused shape')


# ----------------------------------------------------------------------------------------------- boundary merge chain
MC_ROWS = 16                       # output rows of a workgroup band (pointwise.hip)


def _merge_chain_lds_bytes(S):
    return 4 * (2 * S * S + (MC_ROWS // 2 + 5) * 2 * S * 2)      # dm_boundary_merge_chain's LDS request


def _merge_chain_max_s():
    S = 2
    while _merge_chain_lds_bytes(S + 1) <= 64 * 1024:
        S += 1
    return S


def _merge_inputs(n, S, seed):
    """Logits with large regions away from any boundary (smooth blobs) on some RoIs and salt-and-pepper on others."""
    gen = _g(seed)
    a = torch.randn(n, 1, S, S, generator=gen) * 2
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing='ij')
    for i in range(0, n, 2):
        c = torch.rand(2, generator=gen) - 0.5
        a[i, 0] = 4.0 * (0.5 - ((yy - c[0]) ** 2 + (xx - c[1]) ** 2).sqrt()) + 0.1 * a[i, 0]
    a[0, 0, :2, :2] = 0.0                                          # exact ties of the sigmoid threshold
    b = torch.randn(n, 1, 2 * S, 2 * S, generator=gen) * 2
    fin = torch.randn(n, 1, 2 * S, 2 * S, generator=gen) * 2
    return a, b, fin


def _assert_merge_close(got, a, b, fine, S):
    ref = ref_model.boundary_merge([None, a.double(), b.double(), fine.double()])
    bad = (got.cpu().double() - ref).abs() > 1e-4 + 1e-4 * ref.abs()
    assert bad.double().mean() < 2e-3, (S, float(bad.double().mean()))   # (threshold ties of |logit| ~ 1e-7 may flip a 3x3 block)


def test_boundary_merge_chain_lds_limit_is_where_the_formula_puts_it(ops):
    S_max = _merge_chain_max_s()
    assert S_max >= 56
    for S, ok in ((S_max, True), (S_max + 1, False)):
        p1, p2, fin = _dev(torch.zeros(1, 1, S, S)), _dev(torch.zeros(1, 1, 2 * S, 2 * S)), _dev(torch.zeros(1, 1, 2 * S, 2 * S))
        out = _canary(1, 1, 4 * S, 4 * S)
        if ok:
            ops.boundary_merge_chain(p1, p2, fin, out=out)
            continue
        with pytest.raises(RuntimeError, match='not supported'):
            ops.boundary_merge_chain(p1, p2, fin, out=out)
        fine = _canary(1, 1, 4 * S, 4 * S)
        with pytest.raises(RuntimeError, match='not supported'):
            ops.boundary_merge_chain(p1, p2, fine)
        torch.cuda.synchronize()
        _untouched(out, 'out of a refused S')
        _untouched(fine, 'the in-place fine logits of a refused S')


# S from 2 up to the largest the LDS check accepts; 4S not a multiple of the 16-row band at 3, 5, 7, 13; 45 is the largest S
# whose second merge (2S -> 4S) dm_boundary_merge itself still takes
@pytest.mark.parametrize('S,n', [(2, 3), (3, 2), (5, 4), (7, 3), (13, 2), (28, 2), (45, 2), ('max', 2)])
def test_boundary_merge_chain_sweep_has_the_bits_of_its_launches_and_matches_the_oracle(ops, S, n):
    S = _merge_chain_max_s() if S == 'max' else S
    a32, b32, fin32 = _merge_inputs(n, S, 7000 + S)
    a, b, fin = _dev(a32), _dev(b32), _dev(fin32)
    seq_ok = 2 * (2 * S) ** 2 * 4 <= 64 * 1024                     # dm_boundary_merge's own LDS limit at the 2S -> 4S merge
    fine = F.interpolate(fin32, scale_factor=2, mode='bilinear', align_corners=True)
    if seq_ok:
        fine_seq = ops.upsample2x(fin, align_corners=True)
        b_seq = b.clone()
        ops.boundary_merge_(a, b_seq)
        ops.boundary_merge_(b_seq, fine_seq)
    # the form with the final x2 upsample: into rows of a wider buffer, one canary row behind
    buf = _canary(n + 1, 1, 4 * S, 4 * S)
    got = ops.boundary_merge_chain(a, b, fin, out=buf[:n])
    _untouched(buf[n], 'the row behind out')
    assert torch.equal(b, _dev(b32)) and torch.equal(fin, _dev(fin32))     # the 2S inputs are read only
    if seq_ok:
        assert torch.equal(got, fine_seq), S
    _assert_merge_close(got, a32, b32, fine, S)
    # the in-place form on the upsampled fine logits: the same result, the canary row behind them untouched
    fbuf = _canary(n + 1, 1, 4 * S, 4 * S)
    fbuf[:n] = ops.upsample2x(fin, align_corners=True)
    got2 = ops.boundary_merge_chain(a, b, fbuf[:n])
    _untouched(fbuf[n], 'the row behind the in-place fine logits')
    assert torch.equal(got2, got), S


# ----------------------------------------------------------------------------------------------- grouped 1x1 convolutions
# problems (Cin, Cout, H, W): Cin not a multiple of the 16-channel chunk, Cout of one, of a 64-cout tile and a half, of more
# than three; maps smaller than one 128-pixel tile and ragged ones
GROUPS = [
    [(24, 36, 5, 7)],
    [(40, 1, 13, 21), (24, 200, 3, 3)],
    [(24, 200, 9, 14), (40, 36, 1, 1), (256, 1, 11, 12)],
    [(16, 64, 8, 16), (48, 65, 6, 10), (40, 33, 17, 9)],
]


@pytest.mark.parametrize('NB', [1, 3])
@pytest.mark.parametrize('gi', range(len(GROUPS)))
def test_conv1x1_group_sweep_equals_its_own_launches_and_matches_f64(ops, gi, NB):
    probs = GROUPS[gi]
    gen = _g(8000 + 10 * gi + NB)
    xs32 = [torch.randn(NB, cin, h, w, generator=gen) for cin, _, h, w in probs]
    ws32 = [torch.randn(co, cin, 1, 1, generator=gen) / cin ** 0.5 for cin, co, _, _ in probs]
    bs32 = [torch.randn(co, generator=gen) for _, co, _, _ in probs]
    if len(probs) > 1:
        bs32[1] = None                                            # a problem without bias
    xs, wq = [_dev(x) for x in xs32], [ops.pack_conv_weight(_dev(w)) for w in ws32]
    bs = [None if b is None else _dev(b) for b in bs32]
    couts = [co for _, co, _, _ in probs]
    for relu in (True, False):
        bufs = [_canary(NB + 1, co, h, w) for _, co, h, w in probs]
        got = ops.conv1x1_group(xs, wq, bs, couts, relu=relu, outs=[b_[:NB] for b_ in bufs])
        for i, (g_, b_) in enumerate(zip(got, bufs)):
            _untouched(b_[NB], f'the row behind problem {i}')
            assert torch.equal(g_, ops.conv2d(xs[i], wq[i], bs[i], couts[i], 1, relu=relu)), (gi, NB, i, relu)
            r64 = F.conv2d(xs32[i].double(), ws32[i].double(), None if bs32[i] is None else bs32[i].double())
            r32 = F.conv2d(xs32[i], ws32[i], bs32[i])
            if relu:
                r64, r32 = F.relu(r64), F.relu(r32)
            assert_close_via_f64(g_, r32, r64, f'group {gi} problem {i} NB={NB} relu={relu}')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_conv1x1_group_on_the_shared_launcher_equals_lone_conv2d(ops, precision):
    """dm_conv1x1_group_fwd goes through the grouped launcher every grouped entry point uses (its geometry, LDS size and
    grid ranges are no longer set up by hand): for 1, 2 and 3 problems of different shapes -- Cin that is no multiple of
    the 16-channel chunk, Cout of one 64-cout tile and a bit, of exactly one, and of three (the last ragged), maps of
    less and more than one 128-pixel tile -- every output has the bits of its own lone conv2d, in the exact and in the
    bf16x3 layout.  The sweep above already holds the exact layout to this; what this test adds is the bf16x3 layout
    (held elsewhere for three problems of one image only) and every problem leading a group."""
    NB, probs = 3, [(20, 33, 7, 9), (16, 64, 14, 14), (40, 130, 3, 5)]
    gen = _g(8200)
    xs = [_dev(torch.randn(NB, cin, h, w, generator=gen)) for cin, _, h, w in probs]
    wq = [ops.pack_conv_weight(_dev(torch.randn(co, cin, 1, 1, generator=gen) / cin ** 0.5), precision=precision) for cin, co, _, _ in probs]
    bs = [_dev(torch.randn(co, generator=gen)) for _, co, _, _ in probs]
    couts = [co for _, co, _, _ in probs]
    lone = [ops.conv2d(x, q, b, co, 1, relu=True) for x, q, b, co in zip(xs, wq, bs, couts)]
    for k in (1, 2, 3):
        for first in range(0, 3 - k + 1):                       # every problem leads a group once
            sl = slice(first, first + k)
            got = ops.conv1x1_group(xs[sl], wq[sl], bs[sl], couts[sl], relu=True)
            assert len(got) == k
            for g_, r_ in zip(got, lone[sl]):
                assert torch.equal(g_, r_), (precision, k, first)


def test_conv1x1_group_refuses_bad_counts_and_oversized_maps(ops):
    """The entry point's own refusals (ops.conv1x1_group asserts 1 <= count <= 3 before it gets there): nothing written."""
    from dynamask_amd._lib import lib
    x = _dev(torch.randn(1, 16, 4, 4, generator=_g(8100)))
    wq = ops.pack_conv_weight(_dev(torch.randn(8, 16, 1, 1, generator=_g(8101))))
    out = _canary(1, 8, 4, 4)
    stream = ops._stream()
    for count, H, W in ((0, 4, 4), (4, 4, 4), (1, 65536, 65536)):
        ptrs = lambda t: (ctypes.c_void_p * 4)(*([t.data_ptr()] * 4))      # noqa: E731
        ints = lambda v: (ctypes.c_int * 4)(*([v] * 4))                     # noqa: E731
        rc = lib().dm_conv1x1_group_fwd(count, ptrs(x), ints(16), ints(H), ints(W), 1, ptrs(wq), (ctypes.c_void_p * 4)(),
                                        ints(8), 1, ptrs(out), stream)
        assert rc != 0 and 'invalid argument' in lib().dm_error_string(rc).decode(), (count, H, W)
    torch.cuda.synchronize()
    _untouched(out, 'out of a refused group')


# ----------------------------------------------------------------------------------------------- 64-bit addressing of the 1x1s
def test_conv1x1_past_4gb_of_input_takes_the_64bit_path_and_keeps_its_bits(ops):
    """dm_conv2d_fwd and dm_conv1x1_group_fwd turn the 32-bit pixel offsets of their 1x1 staging off once a source spans
    4 GB (NB * Cin * H * W * 4 >= 2^32).  1340 RoIs of 256 x 56 x 56 are 4.3 GB: the last rows lie past 2^32 bytes and must
    have the bits of the same convolution launched on those rows alone (which takes the 32-bit path) and match float64."""
    NB, Cin, S, Cout = 1340, 256, 56, 64
    assert NB * Cin * S * S * 4 >= 1 << 32
    gdev = torch.Generator(device='cuda').manual_seed(9000)
    x = torch.randn(NB, Cin, S, S, device='cuda', generator=gdev)
    w32 = torch.randn(Cout, Cin, 1, 1, generator=_g(9001)) / Cin ** 0.5
    b32 = torch.randn(Cout, generator=_g(9002))
    wq, b = ops.pack_conv_weight(_dev(w32)), _dev(b32)
    try:
        big = ops.conv2d(x, wq, b, Cout, 1, relu=True)
        grp = ops.conv1x1_group([x], [wq], [b], [Cout], relu=True)[0]
        assert torch.equal(grp, big)
        for lo, hi in ((NB - 3, NB), (0, 1)):
            small = ops.conv2d(x[lo:hi].contiguous(), wq, b, Cout, 1, relu=True)
            assert torch.equal(big[lo:hi], small), (lo, hi)
            assert torch.equal(grp[lo:hi], ops.conv1x1_group([x[lo:hi].contiguous()], [wq], [b], [Cout], relu=True)[0])
        tail = x[NB - 3:].cpu()
        r64 = F.relu(F.conv2d(tail.double(), w32.double(), b32.double()))
        r32 = F.relu(F.conv2d(tail, w32, b32))
        assert_close_via_f64(big[NB - 3:], r32, r64, '1x1 past 4 GB')
    finally:
        del x
        big = grp = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
