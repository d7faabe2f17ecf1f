"""deform_conv_c256_kernel: the 14 x 14 DCN with every one of its 256 output channels in one workgroup (256 couts x 64
flat pixels, four waves that own 64 couts each and read their weights from global memory).  It takes the launches of
maps with 128 <= H*W <= 256 and 225..256 output channels from the batch size on at which the 64 x 64 tiles stop -- which
batch that is, and where a launch is cut in two, the tests ask the launcher (ops.deform_conv_plan: its own route; 38 RoIs
of 14 x 14 on 256 CUs).
Every variant of the DCN forms the same products in the same order, so its rows are compared bit for bit with those
of launches small enough for the 64 x 64 kernel, and with the float64 oracle through the fp64 triangle."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

C = 256
SMALL = 16            # RoIs per reference launch: far below every threshold here


def _g(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _plan(ops, n, H, W, cout=C):
    return ops.deform_conv_plan(n, C, H, W, cout, 1)


def _is_64x64(rec):
    return (rec['kernel'], rec['P0'], rec['P1'], rec['P2'], rec['P3']) == (0, 2, 2, 1, 1)


def _threshold(ops, H, W, cout=C):
    """Smallest batch the launcher gives to the c256 kernel (no workspace); SMALL and 3 RoIs take the 64 x 64 build."""
    n = 1
    while ops.DCN_KERNELS[_plan(ops, n, H, W, cout)[0]['kernel']] != 'c256':
        n += 1
    for small in (SMALL, 3):
        one, = _plan(ops, small, H, W, cout)
        assert _is_64x64(one) and one['ksplit'] == 1
    assert n > SMALL
    return n


def _inputs(N, H, W, dg, cout=C, seed=0):
    x = torch.randn(N, C, H, W, generator=_g(900 + seed))
    off = torch.randn(N, 18 * dg, H, W, generator=_g(901 + seed)) * 1.5
    off[0, :, 0, 0] = 40.0                       # far outside: all taps void
    off[-1, ::2, H // 2] = 25.0                  # a row of pixels looks 25 rows down / up: clamps at the borders
    off[-1, ::2, H // 2 + 1] = -25.0
    off[-1, :, -1, -1] = -3.25
    w = torch.randn(cout, C, 3, 3, generator=_g(902 + seed)) / (9 * C) ** 0.5
    return x, off, w


def _by_small_launches(ops, x, off, wq, cout, dg, relu):
    return torch.cat([ops.deform_conv(x[s:s + SMALL].contiguous(), off[s:s + SMALL].contiguous(), wq, cout, dg, relu=relu)
                      for s in range(0, x.shape[0], SMALL)])


@pytest.mark.parametrize('dg', [1, 2, 4])
@pytest.mark.parametrize('H,W', [(14, 14), (16, 16), (11, 12)])
def test_c256_rows_have_the_bits_of_the_64x64_kernel_and_match_f64(ops, H, W, dg):
    """Batches at the threshold and one above it (H*W = 196 and 132: not multiples of the 64-pixel tile, so tiles span two
    images and the last tile is ragged; 256: the LDS maximum, tiles end with the image), deformable groups 1, 2 and 4: EVERY
    row equals the row of a 16-RoI launch, the first rows those of a 3-RoI launch; the first and the last RoI (void
    taps, border clamps) against the oracle in float64, and with zero offsets against F.conv2d."""
    T = _threshold(ops, H, W)
    x, off, w = _inputs(T + 1, H, W, dg)
    xd, offd = x.cuda(), off.cuda()
    wq = ops.pack_conv_weight(w.cuda())
    for N in (T, T + 1):
        big = ops.deform_conv(xd[:N].contiguous(), offd[:N].contiguous(), wq, C, dg, relu=True)
        assert torch.equal(big, _by_small_launches(ops, xd[:N], offd[:N], wq, C, dg, True)), (H, W, dg, N)
        assert torch.equal(big[:3], ops.deform_conv(xd[:3].contiguous(), offd[:3].contiguous(), wq, C, dg, relu=True))
    plain = ops.deform_conv(xd, offd, wq, C, dg)
    assert torch.equal(torch.relu(plain), big)
    sel = [0, T]
    r32 = ref_ops.deform_conv2d(x[sel], off[sel], w, 1, 1, 1, dg)
    r64 = ref_ops.deform_conv2d(x[sel].double(), off[sel].double(), w.double(), 1, 1, 1, dg)
    assert_close_via_f64(plain[sel].cpu(), r32, r64, name=f'dcn c256 {H}x{W} dg={dg}')
    zero = ops.deform_conv(xd, torch.zeros_like(offd), wq, C, dg)
    assert_close_via_f64(zero[sel].cpu(), F.conv2d(x[sel], w, padding=1), F.conv2d(x[sel].double(), w.double(), padding=1),
                         name=f'dcn c256 zero offsets {H}x{W} dg={dg}')


def test_c256_last_round_goes_to_a_second_launch_with_the_same_bits(ops):
    """From one full round of workgroups on (two per compute unit) the tiles of a nearly empty last round run as a
    second launch of 64 x 64 tiles that starts in the middle of the batch: the smallest such batch of 14 x 14 maps,
    rows from the first tile, around the seam and from the end against small launches."""
    H = W = 14
    N = _threshold(ops, H, W)
    while len(_plan(ops, N, H, W)) != 2:
        N += 1
    main, tail = _plan(ops, N, H, W)
    assert ops.DCN_KERNELS[main['kernel']] == 'c256' and _is_64x64(tail)
    assert main['q_begin'] == 0 and main['Q'] == tail['q_begin'] and tail['Q'] == N * H * W
    x, off, w = _inputs(N, H, W, 2, seed=10)
    xd, offd = x.cuda(), off.cuda()
    wq = ops.pack_conv_weight(w.cuda())
    big = ops.deform_conv(xd, offd, wq, C, 2, relu=True)
    seam = tail['q_begin'] // (H * W)                     # the RoI the second launch starts in
    for lo in (0, max(0, seam - 8), N - SMALL):
        hi = min(N, lo + SMALL)
        assert torch.equal(big[lo:hi], ops.deform_conv(xd[lo:hi].contiguous(), offd[lo:hi].contiguous(), wq, C, 2, relu=True)), lo


@pytest.mark.parametrize('H,W', [(14, 14), (11, 12)])
def test_c256_stores_nothing_outside_its_rows(ops, H, W):
    """250 output channels are packed to 256 rows: the six padding rows are computed and never stored.  The output
    lies between two guard RoIs inside one allocation; the rows themselves equal those of small launches (a store
    of a padding row would land in the next RoI's first channels)."""
    cout, dg = 250, 2
    assert ops.packed_cout(cout) == 256
    N = _threshold(ops, H, W, cout) + 1
    x, off, w = _inputs(N, H, W, dg, cout=cout, seed=20)
    xd, offd = x.cuda(), off.cuda()
    wq = ops.pack_conv_weight(w.cuda())
    buf = torch.full((N + 2, cout, H, W), -777.0, device='cuda')
    out = buf[1:N + 1]
    ops.deform_conv(xd, offd, wq, cout, dg, relu=True, out=out)
    assert bool((buf[0] == -777.0).all()) and bool((buf[N + 1] == -777.0).all())
    assert torch.equal(out, _by_small_launches(ops, xd, offd, wq, cout, dg, True))
    sel = [0, N - 1]
    r32 = F.relu(ref_ops.deform_conv2d(x[sel], off[sel], w, 1, 1, 1, dg))
    r64 = F.relu(ref_ops.deform_conv2d(x[sel].double(), off[sel].double(), w.double(), 1, 1, 1, dg))
    assert_close_via_f64(out[sel].cpu(), r32, r64, name=f'dcn c256 cout=250 {H}x{W}')
