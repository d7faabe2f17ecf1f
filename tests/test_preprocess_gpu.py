"""``ops.preprocess_u8`` (dm_preprocess_u8_fwd) against a numpy restatement of dynamask_hip.h section K33 written here
(int64 up to the byte, float32 for the normalisation): every output element in bits, the padding included, ``out``
pre-filled with NaN.  The per-axis table below is a scalar loop of its own, not ``ops.resize_axis_table``."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN = [123.675, 116.28, 103.53]
STD = [58.395, 57.12, 57.375]
FLIPS = (None, 'horizontal', 'vertical')


def _axis(n_src, n_dst):
    rows = []
    for d in range(n_dst):
        f = np.float32((d + 0.5) * (1.0 / (n_dst / n_src)) - 0.5)
        i = int(math.floor(float(f)))
        t = np.float32(f - np.float32(i))
        if i < 0:
            i, t = 0, np.float32(0)
        if i >= n_src - 1:
            i, t = n_src - 1, np.float32(0)
        c0 = int(np.rint(np.float32(np.float32(1) - t) * np.float32(2048)))
        c1 = int(np.rint(t * np.float32(2048)))
        rows.append((i, min(i + 1, n_src - 1), c0, c1))
    return np.array(rows, dtype=np.int64)


def _resized(src, nh, nw):
    """[h, w, 3] uint8 -> [nh, nw, 3] int64 in 0..255: the fixed-point bilinear of K33."""
    h, w = src.shape[:2]
    S = src.astype(np.int64)
    tx, ty = _axis(w, nw), _axis(h, nh)
    r = S[:, tx[:, 0], :] * tx[:, 2][None, :, None] + S[:, tx[:, 1], :] * tx[:, 3][None, :, None]       # [h, nw, 3]
    top, bot = r[ty[:, 0]], r[ty[:, 1]]
    b0, b1 = ty[:, 2][:, None, None], ty[:, 3][:, None, None]
    v = (((b0 * (top >> 4)) >> 16) + ((b1 * (bot >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255)


def _norm(v, to_rgb):
    """[nh, nw, 3] bytes -> [3, nh, nw] float32: (float(v) - mean) * stdinv, two roundings."""
    mean = np.asarray(MEAN, dtype=np.float32)
    stdinv = (1.0 / np.asarray(STD, dtype=np.float64)).astype(np.float32)
    if to_rgb:
        v = v[..., ::-1]
    x = (v.astype(np.float32) - mean).astype(np.float32) * stdinv
    return np.ascontiguousarray(x.astype(np.float32).transpose(2, 0, 1))


def _reference(srcs, sizes, flip, to_rgb, pad):
    out = np.zeros((len(srcs), 3, pad[0], pad[1]), dtype=np.float32)
    for b, (s, (nh, nw)) in enumerate(zip(srcs, sizes)):
        v = _resized(s, nh, nw)
        if flip == 'horizontal':
            v = v[:, ::-1]
        elif flip == 'vertical':
            v = v[::-1]
        out[b, :, :nh, :nw] = _norm(v, to_rgb)
    return out


def _pad(sizes, d=32):
    return max(-(-nh // d) * d for nh, _ in sizes), max(-(-nw // d) * d for _, nw in sizes)


def _run(srcs_dev, sizes, flip, to_rgb, pad):
    from dynamask_amd import ops
    out = torch.full((len(srcs_dev), 3, pad[0], pad[1]), float('nan'), device='cuda')
    stdinv = (1.0 / np.asarray(STD, dtype=np.float64)).astype(np.float32)
    got = ops.preprocess_u8(srcs_dev, sizes, [flip] * len(srcs_dev), np.asarray(MEAN, dtype=np.float32), stdinv, to_rgb, pad,
                            out=out)
    assert got is out
    return out.cpu().numpy()


def _images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f'{int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}'


# name -> (source shapes, resized sizes)
CASES = {
    'one_pixel': ([(1, 1)], [(1, 1)]),
    'upscale_5x7': ([(5, 7)], [(11, 13)]),              # both edge clamps
    'downscale_64x48': ([(64, 48)], [(23, 17)]),
    'identity_37x53': ([(37, 53)], [(37, 53)]),
    'batch_of_two': ([(37, 53), (20, 64)], [(50, 72), (27, 86)]),     # pads 64 x 96 and 32 x 96: zeros below the second
}


@pytest.mark.parametrize('flip', FLIPS)
@pytest.mark.parametrize('to_rgb', [True, False])
@pytest.mark.parametrize('case', sorted(CASES))
def test_bits_of_every_element(case, to_rgb, flip):
    shapes, sizes = CASES[case]
    srcs = _images(shapes, seed=len(case))
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    pad = _pad(sizes)
    got = _run(dev, sizes, flip, to_rgb, pad)
    _same_bits(got, _reference(srcs, sizes, flip, to_rgb, pad))
    for s, d in zip(srcs, dev):
        assert np.array_equal(d.cpu().numpy(), s)               # the sources are only read
    if case == 'batch_of_two':
        assert (got[1, :, 27:, :] == 0).all() and (got[1, :, :, 86:] == 0).all() and (got[0, :, 50:, :] == 0).all()


@pytest.mark.parametrize('flip', FLIPS)
@pytest.mark.parametrize('to_rgb', [True, False])
def test_no_resize_passes_the_bytes_through(to_rgb, flip):
    """nh == h and nw == w: the source byte exactly, so the result is (src - mean) * stdinv with no table involved."""
    src = _images([(37, 53)], seed=3)[0]
    got = _run([torch.from_numpy(src).cuda()], [(37, 53)], flip, to_rgb, (64, 64))
    v = src.astype(np.int64)
    v = v[:, ::-1] if flip == 'horizontal' else v[::-1] if flip == 'vertical' else v
    want = np.zeros((1, 3, 64, 64), dtype=np.float32)
    want[0, :, :37, :53] = _norm(v, to_rgb)
    _same_bits(got, want)


@pytest.mark.parametrize('flip', FLIPS)
@pytest.mark.parametrize('to_rgb', [True, False])
def test_non_contiguous_row_stride(to_rgb, flip):
    wide = _images([(19, 40)], seed=5)[0]
    wide_dev = torch.from_numpy(wide).cuda()
    view = wide_dev[:, 4:27]                                   # 23 columns of 40: row stride 120 bytes
    assert not view.is_contiguous() and view.stride() == (120, 3, 1)
    src = np.ascontiguousarray(wide[:, 4:27])
    sizes = [(31, 29)]
    got = _run([view], sizes, flip, to_rgb, _pad(sizes))
    _same_bits(got, _reference([src], sizes, flip, to_rgb, _pad(sizes)))
    assert np.array_equal(wide_dev.cpu().numpy(), wide)


@pytest.mark.parametrize('value', [0, 255])
def test_constant_images_stay_constant(value):
    """The clamps, and c0 + c1 == 2048 on both axes: an all-255 (all-0) image is all 255 (0) after any resize."""
    for (h, w), (nh, nw) in [((5, 7), (11, 13)), ((64, 48), (23, 17)), ((37, 53), (50, 72))]:
        src = np.full((h, w, 3), value, dtype=np.uint8)
        pad = _pad([(nh, nw)])
        got = _run([torch.from_numpy(src).cuda()], [(nh, nw)], None, True, pad)
        want = np.zeros((1, 3) + pad, dtype=np.float32)
        want[0, :, :nh, :nw] = _norm(np.full((nh, nw, 3), value, dtype=np.int64), True)
        _same_bits(got, want)


def test_an_image_does_not_depend_on_its_batch():
    shapes, sizes = CASES['batch_of_two']
    srcs = _images(shapes, seed=9)
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    both = _run(dev, sizes, 'horizontal', True, _pad(sizes))
    for b in range(2):
        alone = _run([dev[b]], [sizes[b]], 'horizontal', True, _pad([sizes[b]]))
        nh, nw = sizes[b]
        _same_bits(np.ascontiguousarray(both[b, :, :nh, :nw]), np.ascontiguousarray(alone[0, :, :nh, :nw]))


def test_unsupported_input_raises_with_the_code():
    from dynamask_amd import ops
    img = torch.zeros((4, 4, 3), dtype=torch.uint8, device='cuda')
    mean, stdinv = np.zeros(3, np.float32), np.ones(3, np.float32)
    with pytest.raises(RuntimeError, match=r'code -3'):
        ops.preprocess_u8([img], [(0, 4)], [None], mean, stdinv, True, (32, 32))             # n_dst < 1
    with pytest.raises(RuntimeError, match=r'code -3'):
        ops.preprocess_u8([img], [(40, 4)], [None], mean, stdinv, True, (32, 32))            # does not fit the padded output
    with pytest.raises(RuntimeError, match=r'code -3'):
        ops.preprocess_u8([img] * (ops.PREPROCESS_MAX_IMAGES + 1), [(4, 4)] * (ops.PREPROCESS_MAX_IMAGES + 1),
                          [None] * (ops.PREPROCESS_MAX_IMAGES + 1), mean, stdinv, True, (32, 32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.preprocess_u8([img.cpu()], [(4, 4)], [None], mean, stdinv, True, (32, 32))
    with pytest.raises(TypeError, match='uint8'):
        ops.preprocess_u8([img.float()], [(4, 4)], [None], mean, stdinv, True, (32, 32))
    with pytest.raises(ValueError, match='dense pixels'):
        ops.preprocess_u8([img[:, ::2]], [(4, 2)], [None], mean, stdinv, True, (32, 32))
