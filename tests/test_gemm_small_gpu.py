"""dm_deconv2x2_fwd, dm_fc_fwd and the weight packers at the shapes where a GEMM kernel goes wrong -- ragged K chunks,
partly filled tiles in both dimensions, tiles that span several images, no bias -- against float64 (the project's
triangle, tolerances.assert_close_via_f64) and, for the packers, against a numpy restatement of the documented layout.
Every output lies between guard bands filled with a canary."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

CANARY = -7.25
GUARD = 1024
vp = ctypes.c_void_p


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _lib():
    from dynamask_amd._lib import lib
    return lib()


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _banded(numel):
    buf = torch.full((2 * GUARD + numel,), CANARY, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _bands_intact(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


# ------------------------------------------------------------------ deconv 2x2 / s2
DECONV_CH = [(256, 256), (24, 8), (20, 5), (40, 33), (8, 1)]          # 4 * Cout = 20 / 132: ragged CoutP / ragged 128-cout tile
DECONV_MAPS = [(14, 14), (7, 9), (1, 5), (33, 2)]
DECONV_CASES = []
for _i, (_c, _co) in enumerate(DECONV_CH):
    for _j, (_h, _w) in enumerate(DECONV_MAPS):
        _nb = (1, 3, 'many')[(_i + _j) % 3]
        if _nb == 'many':
            _nb = -(-300 // (_h * _w)) if _h * _w < 64 else 3       # more than two images in a 128-pixel tile where the map allows
        DECONV_CASES.append((_c, _co, _h, _w, _nb, (_i + _j) % 2 == 0, (_i + 2 * _j) % 3 != 0))
DECONV_CASES.append((20, 5, 1, 5, 61, True, True))                     # 305 pixels: tiles of 25.6 images, a ragged third tile
DECONV_CASES.append((40, 33, 7, 9, 7, False, True))                    # 441 pixels: tiles that start inside an image


@pytest.mark.parametrize('C,cout,H,W,NB,bias,relu', DECONV_CASES)
def test_deconv2x2_against_float64(ops, C, cout, H, W, NB, bias, relu):
    x = torch.randn(NB, C, H, W, generator=_g(C + cout))
    w = torch.randn(C, cout, 2, 2, generator=_g(C + cout + 1)) / C ** 0.5
    b = torch.randn(cout, generator=_g(C + cout + 2)) if bias else None
    wq = ops.pack_deconv_weight(w.cuda())
    buf, flat = _banded(NB * cout * 4 * H * W)
    xd, bd = x.cuda(), None if b is None else b.cuda()
    rc = _lib().dm_deconv2x2_fwd(vp(xd.data_ptr()), NB, C, H, W, vp(wq.data_ptr()), None if bd is None else vp(bd.data_ptr()), cout,
                                 1 if relu else 0, vp(flat.data_ptr()), _stream())
    assert rc == 0
    out = flat.view(NB, cout, 2 * H, 2 * W)
    assert _bands_intact(buf) and not bool((out == CANARY).any()), 'an output was not written / a guard band was'
    r32 = F.conv_transpose2d(x, w, b, stride=2)
    r64 = F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2)
    if relu:
        r32, r64 = r32.relu(), r64.relu()
    assert_close_via_f64(out.cpu(), r32, r64, f'deconv {C}->{cout} {H}x{W} x{NB}')
    assert torch.equal(out, ops.deconv2x2(xd, wq, bd, cout, relu=relu))


# ------------------------------------------------------------------ fully connected
def _fc(x, w, b, relu, refuse=None):
    """dm_fc_fwd with a scratch of exactly dm_fc_scratch_floats floats and a canary behind it, out between guard bands."""
    N, K = x.shape
    M = w.shape[0]
    ns = int(_lib().dm_fc_scratch_floats(N, K, M))
    scratch = torch.full((ns + GUARD,), CANARY, device='cuda')
    buf, flat = _banded(N * M)
    rc = _lib().dm_fc_fwd(vp(x.data_ptr()), vp(w.data_ptr()), None if b is None else vp(b.data_ptr()), N, K, M, 1 if relu else 0,
                          vp(flat.data_ptr()), vp(scratch.data_ptr()) if ns else None, _stream())
    torch.cuda.synchronize()
    assert bool((scratch[ns:] == CANARY).all()), 'wrote past dm_fc_scratch_floats'
    assert _bands_intact(buf)
    if refuse is not None:
        assert rc == refuse and bool((flat == CANARY).all()) and bool((scratch == CANARY).all())
        return None
    assert rc == 0
    return flat.view(N, M).clone(), ns


def _splits(K):
    """include/dynamask_hip.h, K22: segments of 256 elements up to K = 4096, of 1024 above."""
    seg = 256 if K <= 4096 else 1024
    return -(-K // seg)


# K: 4 a single partial chunk; 36 a ragged second chunk; 252 / 256 one split of 256, ragged / full; 260 two splits, the
# second a single quad; 4096 / 4100 either side of the segment switch (16 x 256, 5 x 1024 with a one-quad last split);
# 5124: a last 1024-split that holds one quad
FC_CASES = [(1, 4, 1, False, False), (127, 36, 3, True, True), (128, 252, 81, False, True), (129, 256, 128, True, False),
            (257, 260, 129, False, False), (129, 4096, 320, True, True), (127, 4100, 129, False, True), (257, 5124, 81, True, False),
            (1, 5124, 320, False, True), (128, 4, 128, True, True), (257, 36, 320, False, False), (129, 260, 1, True, False),
            (3, 4096, 3, False, False), (128, 4100, 128, True, False)]


@pytest.mark.parametrize('N,K,M,bias,relu', FC_CASES)
def test_fc_against_float64(N, K, M, bias, relu):
    x = torch.randn(N, K, generator=_g(K + N))
    w = torch.randn(M, K, generator=_g(K + M + 1)) / K ** 0.5
    b = torch.randn(M, generator=_g(K + 2)) if bias else None
    out, ns = _fc(x.cuda(), w.cuda(), None if b is None else b.cuda(), relu)
    assert ns == (_splits(K) * N * M if _splits(K) > 1 else 0)
    r32 = F.linear(x, w, b)
    r64 = F.linear(x.double(), w.double(), None if b is None else b.double())
    if relu:
        r32, r64 = r32.relu(), r64.relu()
    assert_close_via_f64(out.cpu(), r32, r64, f'fc N {N} K {K} M {M}')


@pytest.mark.parametrize('K', [4, 36, 252, 256, 260, 4096, 4100, 5124])
def test_fc_rows_do_not_depend_on_n(K):
    M = 129
    x = torch.randn(257, K, generator=_g(K)).cuda()
    w = (torch.randn(M, K, generator=_g(K + 1)) / K ** 0.5).cuda()
    b = torch.randn(M, generator=_g(K + 2)).cuda()
    full, _ = _fc(x, w, b, False)
    for n in (1, 127, 128, 129):
        part, _ = _fc(x[:n].contiguous(), w, b, False)
        assert torch.equal(part, full[:n]), (K, n)
    nobias, _ = _fc(x, w, None, False)
    r64 = F.linear(x.cpu().double(), w.cpu().double())
    assert_close_via_f64(nobias.cpu(), F.linear(x.cpu(), w.cpu()), r64, f'fc K {K} without bias')


@pytest.mark.parametrize('K', [6, 255, 4098])
def test_fc_refuses_k_not_a_multiple_of_4(K):
    x, w = torch.randn(5, K, device='cuda'), torch.randn(7, K, device='cuda')
    _fc(x, w, None, False, refuse=-3)


# ------------------------------------------------------------------ the packers
def _pack_ref(w, srcs, flip):
    """include/dynamask_hip.h: OIHW -> [k*k][KQ][CoutP][4], input channels in quads, every source padded with zero rows to a
    multiple of 8 channels, CoutP = Cout rounded up to 32, zero padded; transpose_flip: channels swapped, taps rotated."""
    w = w.numpy()
    kk = w.shape[2] * w.shape[3]
    w = w.reshape(w.shape[0], w.shape[1], kk)
    m = np.transpose(w[:, :, ::-1], (2, 0, 1)) if flip else np.transpose(w, (2, 1, 0))        # [tap][reduction row][produced col]
    rows, cols = m.shape[1], m.shape[2]
    assert sum(srcs) == rows
    colsP, K = -(-cols // 32) * 32, sum(-(-c // 8) * 8 for c in srcs)
    out = np.zeros((kk, K, colsP), np.float32)
    p = base = 0
    for c in srcs:
        out[:, p:p + c, :cols] = m[:, base:base + c]
        p, base = p + -(-c // 8) * 8, base + c
    return out.reshape(kk, K // 4, 4, colsP).transpose(0, 1, 3, 2).reshape(-1)


PACK_CASES = [(ks, srcs, cout, flip) for ks in (1, 3) for srcs in ([20], [24, 8, 1, 1]) for cout in (30, 65, 130) for flip in (False, True)]


@pytest.mark.parametrize('ks,srcs,cout,flip', PACK_CASES)
def test_pack_weight_layout(ops, ks, srcs, cout, flip):
    red = sum(srcs)
    w = torch.randn((red, cout, ks, ks) if flip else (cout, red, ks, ks), generator=_g(red + cout + ks))
    assert float(w.abs().min()) > 0                                                  # zeros below are padding, nothing else
    n = ops.packed_floats(cout, ks, srcs)
    buf, flat = _banded(n)
    wd = w.cuda()
    rc = _lib().dm_conv_pack_weight(vp(wd.data_ptr()), w.shape[0], w.shape[1], ks, 1 if flip else 0, len(srcs),
                                    (ctypes.c_int * len(srcs))(*srcs), vp(flat.data_ptr()), _stream())
    assert rc == 0 and _bands_intact(buf)
    ref = _pack_ref(w, srcs, flip)
    assert ref.size == n
    assert np.array_equal(flat.cpu().numpy(), ref)


def test_pack_weight_batch_window_gives_the_bits_of_the_sliced_pack(ops):
    """dm_conv_pack_weight_batch: a job whose [Cout][Cin] tensor is the input-channel window [c0, c0 + Cin) of a
    [Cout][ld][k][k] tensor (ld > Cin, c0 > 0) packs what dm_conv_pack_weight packs of the sliced tensor."""
    from dynamask_amd._lib import PackJob
    jobs, keep = [], []
    #        O    ld  c0  Cin ks flip  srcs (sum: Cin, or O under flip)
    spec = [(30, 50, 7, 34, 3, 0, [24, 8, 1, 1]), (65, 41, 1, 20, 1, 0, [20]), (34, 130, 65, 65, 3, 1, [24, 8, 1, 1]),
            (20, 33, 3, 30, 1, 1, [20]), (130, 20, 0, 20, 3, 0, [20])]
    for i, (O, ld, c0, cin, ks, flip, srcs) in enumerate(spec):
        wide = torch.randn(O, ld, ks, ks, generator=_g(50 + i))
        cols = cin if flip else O
        n = ops.packed_floats(cols, ks, srcs)
        buf, flat = _banded(n)
        wd = wide.cuda()
        single = ops.pack_conv_weight(wide[:, c0:c0 + cin].contiguous().cuda(), transpose_flip=bool(flip), src_channels=srcs)
        assert np.array_equal(single.cpu().numpy(), _pack_ref(wide[:, c0:c0 + cin].contiguous(), srcs, bool(flip)))
        jobs.append((wd, flat, O, cin, ks, flip, srcs, ld, c0))
        keep.append((buf, flat, single))
    arr = (PackJob * len(jobs))()
    for j, (wd, flat, O, cin, ks, flip, srcs, ld, c0) in zip(arr, jobs):
        j.w, j.w_packed = wd.data_ptr(), flat.data_ptr()
        j.Cout, j.Cin, j.ksize, j.transpose_flip, j.num_srcs = O, cin, ks, flip, len(srcs)
        for k, c in enumerate(srcs):
            j.src_channels[k] = c
        j.ld, j.c0 = ld, c0
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    assert _lib().dm_conv_pack_weight_batch(vp(table.data_ptr()), len(jobs), _stream()) == 0
    torch.cuda.synchronize()
    for i, (buf, flat, single) in enumerate(keep):
        assert _bands_intact(buf), i
        assert torch.equal(flat, single), f'job {i}'
