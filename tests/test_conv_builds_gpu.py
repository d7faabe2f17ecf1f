"""Every tile build of the exact-fp32 convolution launcher (csrc/conv_igemm.hip: conv2d_launch) against float64.

Each case first asks the launcher for its plan (ops.conv2d_plan: the launcher's own report, nothing restated here) and
asserts the build it was written for; NB is derived from the workgroup count the case wants and the device's
compute-unit count.  Then the launch is compared with F.conv2d of the same fp32 inputs in float64 on the CPU through
the project's triangle (tolerances.assert_close_via_f64: rel 1e-4, the fp32 torch result as the third corner), `out` is
a channel slice of a wider tensor inside a buffer with guard bands, and every canary must be intact.  Shapes are the
smallest with more than one K chunk, a ragged last chunk and a partly filled last tile in both dimensions.

TABLE lists every reachable (build, MAXPOS) pair of the exact launcher; test_every_build_is_reached holds the sweep to
it.  Out of scope here: the bf16x3 builds (PREC 1: tests/test_precision_gpu.py) and the post-add builds (POST 1:
tests/test_htc_gpu.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

KEYS = ('KS', 'WGM', 'WGN', 'WM', 'WN', 'CK', 'TAIL')
B128, B32, B64, B32C, BTAIL = (3, 2, 2, 2, 2, 8, 0), (3, 4, 1, 1, 1, 8, 0), (3, 1, 4, 2, 1, 8, 0), (3, 1, 4, 1, 1, 8, 0), (3, 1, 4, 1, 1, 8, 4)
P1_SMALL, P1_128, P1_64, P1_32 = (1, 4, 1, 1, 1, 32, 0), (1, 2, 2, 2, 2, 16, 0), (1, 2, 2, 1, 2, 16, 0), (1, 1, 4, 1, 1, 32, 0)
NAMES = {B128: '3x3 128x128', B32: '3x3 128x32', B64: '3x3 64x128', B32C: '3x3 32x128', BTAIL: '3x3 32+4x128',
         P1_SMALL: '1x1 128x32 ck32', P1_128: '1x1 128x128', P1_64: '1x1 64x128', P1_32: '1x1 32x128'}
# every (build, MAXPOS) the exact fp32 launcher can produce (PREC = POST = 0)
TABLE = {(b, mp) for b in (B128, B32, B64, B32C, BTAIL) for mp in (1, 2, 4)} | {(b, 1) for b in (P1_SMALL, P1_128, P1_64, P1_32)}
CANARY = -7.25
GUARD = 4096
ERRS = {}           # (build, MAXPOS) -> [largest |product - f64|, the fp32 reference's own error] over the cases that ran


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


CUS = _cus()


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _plan(srcs, NB, H, W, cout, ks, **kw):
    from dynamask_amd import ops as o
    return o.conv2d_plan(srcs, NB, H, W, cout, ks, **kw)


def _bm(rec):
    assert rec['PREC'] == 0 and rec['POST'] == 0
    return tuple(rec[k] for k in KEYS), rec['MAXPOS']


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _weights(srcs, cout, ks, seed):
    cin = sum(srcs)
    w = torch.randn(cout, cin, ks, ks, generator=_g(seed)) / (cin * ks * ks) ** 0.5
    b = torch.randn(cout, generator=_g(seed + 1))
    return w, b


def _inputs(srcs, NB, H, W, seed):
    return [torch.randn(NB, c, H, W, generator=_g(seed + 10 + i)) for i, c in enumerate(srcs)]


def _reference(xs, idx, w, b, ks, relu=False, prev=None, mask=None):
    """(fp32, float64) F.conv2d of images idx, with the epilogue in the header's order: + bias, + out (accumulate), ReLU, mask."""
    x = torch.cat([t[idx] for t in xs], 1)
    r32 = F.conv2d(x, w, b, padding=ks // 2)
    r64 = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=ks // 2)
    if prev is not None:
        r32, r64 = r32 + prev[idx], r64 + prev[idx].double()
    if relu:
        r32, r64 = r32.relu(), r64.relu()
    if mask is not None:
        r32, r64 = torch.where(mask[idx] > 0, r32, torch.zeros(())), torch.where(mask[idx] > 0, r64, torch.zeros((), dtype=torch.float64))
    return r32, r64


def _launch(ops, xs_dev, w_dev, b_dev, srcs, cout, ks, variant='plain', seed=0, expect_error=None):
    """One conv2d launch into channels [1, 1 + cout) of a [NB, cout + 3, H, W] tensor between two guard bands, all filled
    with a canary.  Returns (out [NB, cout, H, W], prev, mask) -- prev / mask on the CPU, as the reference needs them."""
    NB, _, H, W = xs_dev[0].shape
    ct = cout + 3
    buf = torch.full((2 * GUARD + NB * ct * H * W,), CANARY, device='cuda')
    out = buf[GUARD:GUARD + NB * ct * H * W].view(NB, ct, H, W)
    prev = mask = None
    kw = {}
    if variant == 'accumulate':
        prev = torch.randn(NB, cout, H, W, generator=_g(seed + 50))
        out[:, 1:1 + cout] = prev.cuda()
        kw['accumulate'] = True
    if variant == 'masked':
        mask = torch.randn(NB, cout, H, W, generator=_g(seed + 51))
        mfull = torch.ones(NB, ct, H, W, device='cuda')
        mfull[:, 1:1 + cout] = mask.cuda()
        kw['mask'] = mfull
    if variant == 'relu':
        kw['relu'] = True
    if variant == 'sliced':
        # the first source is a channel slice of a wider tensor (src_batch_strides)
        c0 = xs_dev[0].shape[1]
        wide = torch.full((NB, c0 + 3, H, W), 1e30, device='cuda')
        wide[:, 2:2 + c0] = xs_dev[0]
        xs_dev = [wide[:, 2:2 + c0]] + list(xs_dev[1:])
        assert not xs_dev[0].is_contiguous() or NB == 1
    wq = ops.pack_conv_weight(w_dev, src_channels=srcs)
    bias = None if variant == 'nobias' else b_dev
    if expect_error is not None:
        with pytest.raises(RuntimeError, match=f'code {expect_error}'):
            ops.conv2d(xs_dev, wq, bias, cout, ks, out=out, out_ch_offset=1, **kw)
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all()), 'a refused launch wrote to out'
        return None, None, None
    if variant == 'overlapped':
        with ops.overlapped_streams():
            ops.conv2d(xs_dev, wq, bias, cout, ks, out=out, out_ch_offset=1, **kw)
    else:
        ops.conv2d(xs_dev, wq, bias, cout, ks, out=out, out_ch_offset=1, **kw)
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all()), 'guard band overwritten'
    assert bool((out[:, 0] == CANARY).all()) and bool((out[:, 1 + cout:] == CANARY).all()), 'neighbouring channels overwritten'
    return out[:, 1:1 + cout].contiguous(), prev, mask


def _images(NB, recs, HW, sample=0):
    """First two, last two, every image a launch boundary touches (and its neighbours), and `sample` evenly spread ones."""
    idx = {0, 1, NB - 2, NB - 1}
    for r in recs[1:]:
        n = r['q_begin'] // HW
        idx |= {(r['q_begin'] - 1) // HW - 1, (r['q_begin'] - 1) // HW, n, n + 1}
    if sample:
        idx |= {int(i) for i in torch.linspace(0, NB - 1, sample).tolist()}
    return sorted(i for i in idx if 0 <= i < NB)


def _hold(out, xs, w, b, ks, idx, recs, name, **epi):
    r32, r64 = _reference(xs, idx, w, b, ks, **epi)
    err, ref_err, _ = assert_close_via_f64(out[idx].cpu(), r32, r64, name)
    print(f'{name}: |product - f64| {err:.3g}, fp32 reference {ref_err:.3g}')
    for r in recs:
        e = ERRS.setdefault(_bm(r), [0.0, 0.0])
        e[0], e[1] = max(e[0], err), max(e[1], ref_err)


# ------------------------------------------------------------------ 3x3, Cout > 64: the 128 x 128 and 128 x 32 builds, the seam
FAMS = {
    # per_cu: workgroups of the 128 x 128 build per CU (three with one staged position per thread, else two);
    # mp128 / mp32: the staged depth of the two builds on this map
    'a': dict(srcs=[20], cout=72, H=14, W=14, per_cu=3, mp128=1, mp32=1),
    'b': dict(srcs=[8, 3, 1], cout=130, H=28, W=28, per_cu=2, mp128=2, mp32=1),
    'c': dict(srcs=[12], cout=65, H=9, W=112, per_cu=2, mp128=4, mp32=4),
    'd': dict(srcs=[16], cout=96, H=2, W=2, per_cu=2, mp128=4, mp32=1),
}
# category -> (what the launch must be, which workgroup counts qualify, which of those to take)
CATS = ('small1', 'small2', 'plain', 'round1', 'seam_min', 'seam_max', 'noseam', 'two_tail')
KIND = dict(small1='small', small2='small', plain='plain', round1='plain', seam_min='seam', seam_max='seam', noseam='plain', two_tail='seam')


def _mt(cout):
    return -(-(-(-cout // 32) * 32) // 128)


def _wgs(f, NB):
    return _mt(f['cout']) * -(-NB * f['H'] * f['W'] // 128)


_PICKS = {}


def _pick(f, cat, cus=CUS):
    """The NB whose 128 x 128 workgroup count lands in the category (None: no batch size of this map does)."""
    key = (f['H'], f['W'], f['cout'], f['per_cu'], cat, cus)
    if key not in _PICKS:
        _PICKS[key] = _search(f, cat, cus)
    return _PICKS[key]


def _search(f, cat, cus):
    # The thresholds below only steer the SEARCH for a batch size; they decide nothing.  Every batch found is then put to
    # the launcher's own plan (_check_kind on ops.conv2d_plan), so a rule that moves in the C++ shows as a failing case.
    slots, HW, mt = f['per_cu'] * cus, f['H'] * f['W'], _mt(f['cout'])
    seam = lambda w: 0 < w % slots and (w % slots) * 5 <= 3 * slots
    rule = {
        'small1': (lambda w: w * 10 <= cus * 7, lambda w: -w),
        'small2': (lambda w: cus < w and w * 20 <= cus * 29, lambda w: -w),
        'plain': (lambda w: w * 20 > cus * 29 and w * 10 > cus * 7 and w < slots, lambda w: abs(w - (cus * 29 // 20 + slots) // 2)),
        'round1': (lambda w: w == slots, lambda w: 0),
        'seam_min': (lambda w: slots < w < 2 * slots and seam(w), lambda w: w),
        'seam_max': (lambda w: slots < w < 2 * slots and seam(w), lambda w: -w),
        'noseam': (lambda w: slots < w < 2 * slots and not seam(w), lambda w: w),
        'two_tail': (lambda w: 2 * slots < w < 3 * slots and seam(w), lambda w: abs(w - 2 * slots - slots // 4)),
    }[cat]
    best = None
    for tiles in range(1, 3 * slots // mt + 1):             # pixel tiles of 128; a batch ends in this tile or none does
        NB = -(-((tiles - 1) * 128 + 1) // HW)
        if NB < 2 or NB * HW > tiles * 128:
            continue
        w = mt * tiles
        if rule[0](w) and (best is None or rule[1](w) < rule[1](_wgs(f, best))):
            best = NB
    return best


WIDE_CASES = [(fam, cat) for fam in FAMS for cat in CATS if _pick(FAMS[fam], cat) is not None]
_FAM = {}


def _family(ops, fam):
    """The family's inputs at its largest batch (two rounds and a tail) and that launch's output, computed once: every other
    case of the family runs on the leading images and must give the same bits."""
    if fam not in _FAM:
        f = FAMS[fam]
        NB = _pick(f, 'two_tail')
        seed = 1000 + 100 * sorted(FAMS).index(fam)
        xs = _inputs(f['srcs'], NB, f['H'], f['W'], seed)
        w, b = _weights(f['srcs'], f['cout'], 3, seed)
        d = dict(f, NB=NB, xs=xs, w=w, b=b, xs_dev=[t.cuda() for t in xs], w_dev=w.cuda(), b_dev=b.cuda())
        recs = _plan(f['srcs'], NB, f['H'], f['W'], f['cout'], 3)
        assert [_bm(r) for r in recs] == [(B128, f['mp128']), (B32, f['mp32'])], recs
        d['big'], _, _ = _launch(ops, d['xs_dev'], d['w_dev'], d['b_dev'], f['srcs'], f['cout'], 3)
        _hold(d['big'], xs, w, b, 3, _images(NB, recs, f['H'] * f['W'], sample=24), recs, f'family {fam} NB {NB} (largest)')
        _FAM[fam] = d
    return _FAM[fam]


def _check_kind(f, recs, kind, NB):
    HW = f['H'] * f['W']
    if kind == 'small':
        assert [_bm(r) for r in recs] == [(B32, f['mp32'])], recs
    elif kind == 'plain':
        assert [_bm(r) for r in recs] == [(B128, f['mp128'])], recs
    else:
        assert [_bm(r) for r in recs] == [(B128, f['mp128']), (B32, f['mp32'])], recs
        assert recs[0]['q_begin'] == 0 and recs[0]['Q'] == recs[1]['q_begin'] and recs[0]['Q'] % 128 == 0 and recs[1]['Q'] == NB * HW
    assert recs[0]['q_begin'] == 0 and recs[-1]['Q'] == NB * HW and all(r['ksplit'] == 1 and r['nontemporal'] == 0 for r in recs)


@pytest.mark.parametrize('fam,cat', WIDE_CASES)
def test_3x3_wide_build_by_workgroup_count(ops, fam, cat):
    if _pick(FAMS[fam], 'two_tail') is None:
        assert CUS != 256
        pytest.skip('no batch size of this map gives the family\'s largest launch on this device')
    d = _family(ops, fam)
    NB = _pick(d, cat)
    recs = _plan(d['srcs'], NB, d['H'], d['W'], d['cout'], 3)
    _check_kind(d, recs, KIND[cat], NB)
    if cat == 'round1':
        assert recs[0]['grid_x'] == d['per_cu'] * CUS
    out, _, _ = _launch(ops, [t[:NB].contiguous() for t in d['xs_dev']], d['w_dev'], d['b_dev'], d['srcs'], d['cout'], 3)
    _hold(out, d['xs'], d['w'], d['b'], 3, _images(NB, recs, d['H'] * d['W'], sample=8), recs, f'family {fam} {cat} NB {NB}')
    assert torch.equal(out, d['big'][:NB]), 'the bits depend on the build / the seam'
    # flag bit 3 removes the seam and leaves the bits
    hinted = _plan(d['srcs'], NB, d['H'], d['W'], d['cout'], 3, overlapped=True)
    assert len(hinted) == 1 and hinted[0]['q_begin'] == 0 and hinted[0]['Q'] == NB * d['H'] * d['W']
    if KIND[cat] == 'seam':
        assert _bm(hinted[0]) == (B128, d['mp128'])
        out2, _, _ = _launch(ops, [t[:NB].contiguous() for t in d['xs_dev']], d['w_dev'], d['b_dev'], d['srcs'], d['cout'], 3, 'overlapped')
        assert torch.equal(out2, out)


def test_a_seam_starts_inside_an_image():
    starts = []
    for fam, cat in WIDE_CASES:
        f = FAMS[fam]
        if KIND[cat] == 'seam':
            recs = _plan(f['srcs'], _pick(f, cat), f['H'], f['W'], f['cout'], 3)
            starts.append(recs[1]['q_begin'] % (f['H'] * f['W']))
    assert any(starts), 'no seam case starts its second launch inside an image'


VARIANTS = ('relu', 'nobias', 'accumulate', 'masked', 'sliced')


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('cat', ['small1', 'seam_min'])
@pytest.mark.parametrize('fam', sorted(FAMS))
def test_3x3_wide_flags(ops, fam, cat, variant):
    NB = _pick(FAMS[fam], cat)
    if NB is None or _pick(FAMS[fam], 'two_tail') is None:
        assert CUS != 256
        pytest.skip('no batch size of this map gives the workgroup count on this device')
    d = _family(ops, fam)
    extra = dict(accumulate=True) if variant == 'accumulate' else dict(has_mask=True) if variant == 'masked' else \
        dict(relu=True) if variant == 'relu' else {}
    if variant == 'sliced':
        extra = dict(src_batch_strides=[(c + (3 if i == 0 else 0)) * d['H'] * d['W'] for i, c in enumerate(d['srcs'])])
    recs = _plan(d['srcs'], NB, d['H'], d['W'], d['cout'], 3, **extra)
    _check_kind(d, recs, KIND[cat], NB)
    xs_dev = [t[:NB].contiguous() for t in d['xs_dev']]
    out, prev, mask = _launch(ops, xs_dev, d['w_dev'], d['b_dev'], d['srcs'], d['cout'], 3, variant, seed=7)
    _hold(out, d['xs'], d['w'], None if variant == 'nobias' else d['b'], 3, _images(NB, recs, d['H'] * d['W'], sample=8), recs,
          f'family {fam} {cat} {variant}', relu=variant == 'relu', prev=prev, mask=mask)
    base = d['big'][:NB]
    if variant == 'relu':
        assert torch.equal(out, base.relu())
    if variant == 'sliced':
        assert torch.equal(out, base)
    if variant == 'masked':
        assert torch.equal(out, torch.where(mask.cuda() > 0, base, torch.zeros((), device='cuda')))


# ------------------------------------------------------------------ 3x3, Cout <= 64
NARROW_MAPS = [((14, 14), 1, 2), ((56, 56), 2, 3), ((5, 120), 4, 2), ((1, 14), 4, 25), ((3, 1), 4, 100)]      # (map, MAXPOS, NB)
NARROW_COUTS = [(33, BTAIL), (36, BTAIL), (37, B64), (64, B64), (1, B32C), (32, B32C)]
NARROW_CASES = []
for _i, (_hw, _mp, _nb) in enumerate(NARROW_MAPS):
    for _j, (_c, _b) in enumerate(NARROW_COUTS):
        _v = ('plain',) + VARIANTS
        _var = _v[(_i + _j) % len(_v)]
        if _b is BTAIL and _var == 'accumulate':
            _var = 'plain'                    # (accumulate on these counts is the next block of cases)
        NARROW_CASES.append((_hw, _mp, _nb, [20] if (_i + _j) % 2 == 0 else [8, 3, 1], _c, _b, _var))
    for _c in (33, 36):
        NARROW_CASES.append((_hw, _mp, _nb, [20], _c, B64, 'accumulate'))


@pytest.mark.parametrize('hw,mp,NB,srcs,cout,build,variant', NARROW_CASES,
                         ids=[f'{h}x{w_}-{c}-{"+".join(map(str, s))}-{v}' for (h, w_), _, _, s, c, _, v in NARROW_CASES])
def test_3x3_narrow_builds(ops, hw, mp, NB, srcs, cout, build, variant):
    H, W = hw
    assert NB * H * W > 256 and NB * H * W % 128 != 0                 # more than one workgroup, a ragged last tile
    extra = dict(accumulate=True) if variant == 'accumulate' else dict(has_mask=True) if variant == 'masked' else {}
    recs = _plan(srcs, NB, H, W, cout, 3, **extra)
    assert [_bm(r) for r in recs] == [(build, mp)], recs
    xs = _inputs(srcs, NB, H, W, 300 + cout)
    w, b = _weights(srcs, cout, 3, 400 + cout)
    out, prev, mask = _launch(ops, [t.cuda() for t in xs], w.cuda(), b.cuda(), srcs, cout, 3, variant, seed=cout)
    _hold(out, xs, w, None if variant == 'nobias' else b, 3, list(range(NB)), recs, f'3x3 {H}x{W} cout {cout} {variant}',
          relu=variant == 'relu', prev=prev, mask=mask)


# ------------------------------------------------------------------ 1x1
P1_MAPS = [(14, 14), (33, 33), (1, 1), (7, 200)]
P1_SRCS = [[40], [72], [24, 8, 1, 1]]
P1_WIDE = [(cout, P1_MAPS[(i + j) % 4], P1_SRCS[(i + 2 * j) % 3]) for i, cout in enumerate((65, 126, 130, 256)) for j in range(4)]


def _p1_nbs(cout, H, W, cus=CUS):
    """(a few images, the last batch at or below (5 cus) / 4 tiles of 128 x 128, the first above, one well above)."""
    mt, HW, thr = _mt(cout), H * W, (5 * cus) // 4
    tiles = lambda NB: mt * -(-NB * HW // 128)
    hi = 1
    while tiles(hi) <= thr:
        hi += 1
    return min(3, hi - 1), hi - 1, hi, hi + max(2, hi // 8)


@pytest.mark.parametrize('cout,hw,srcs', P1_WIDE, ids=[f'{c}-{h}x{w_}-{"+".join(map(str, s))}' for c, (h, w_), s in P1_WIDE])
def test_1x1_wide_builds_on_either_side_of_the_tile_threshold(ops, cout, hw, srcs):
    H, W = hw
    few, last_small, first_big, big = _p1_nbs(cout, H, W)
    xs = _inputs(srcs, big, H, W, 500 + cout)
    w, b = _weights(srcs, cout, 1, 600 + cout)
    xs_dev, w_dev, b_dev = [t.cuda() for t in xs], w.cuda(), b.cuda()
    outs = {}
    for NB, build in ((big, P1_128), (first_big, P1_128), (last_small, P1_SMALL), (few, P1_SMALL)):
        recs = _plan(srcs, NB, H, W, cout, 1)
        assert [_bm(r) for r in recs] == [(build, 1)], (NB, recs)
        out, _, _ = _launch(ops, [t[:NB].contiguous() for t in xs_dev], w_dev, b_dev, srcs, cout, 1)
        _hold(out, xs, w, b, 1, _images(NB, recs, H * W, sample=6), recs, f'1x1 {H}x{W} cout {cout} NB {NB}')
        outs[NB] = out
        assert torch.equal(out, outs[big][:NB]), 'the bits depend on the 1x1 build'
    # flags, on the smaller launch: accumulating and masked launches take the 128 x 128 build whatever their size
    variant = VARIANTS[(cout + H) % len(VARIANTS)]
    extra = dict(accumulate=True) if variant == 'accumulate' else dict(has_mask=True) if variant == 'masked' else {}
    recs = _plan(srcs, few, H, W, cout, 1, **extra)
    assert [_bm(r) for r in recs] == [(P1_128 if extra else P1_SMALL, 1)]
    out, prev, mask = _launch(ops, [t[:few].contiguous() for t in xs_dev], w_dev, b_dev, srcs, cout, 1, variant, seed=cout)
    _hold(out, xs, w, None if variant == 'nobias' else b, 1, list(range(few)), recs, f'1x1 {H}x{W} cout {cout} {variant}',
          relu=variant == 'relu', prev=prev, mask=mask)
    if variant == 'masked':
        assert torch.equal(out, torch.where(mask.cuda() > 0, outs[few], torch.zeros((), device='cuda')))


def _p1_narrow_nb(H, W):
    NB = max(3, -(-300 // (H * W)))             # more than two tiles of 128 pixels, a ragged last one
    return NB + 1 if NB * H * W % 128 == 0 else NB


P1_NARROW = [(cout, build, P1_MAPS[(i + j) % 4], P1_SRCS[(i + j) % 3], (('plain',) + VARIANTS)[(2 * i + j) % 6])
             for i, (cout, build) in enumerate(((33, P1_64), (64, P1_64), (1, P1_32), (32, P1_32))) for j in range(4)]


@pytest.mark.parametrize('cout,build,hw,srcs,variant', P1_NARROW,
                         ids=[f'{c}-{h}x{w_}-{"+".join(map(str, s))}-{v}' for c, _, (h, w_), s, v in P1_NARROW])
def test_1x1_narrow_builds(ops, cout, build, hw, srcs, variant):
    H, W = hw
    NB = _p1_narrow_nb(H, W)
    extra = dict(accumulate=True) if variant == 'accumulate' else dict(has_mask=True) if variant == 'masked' else {}
    recs = _plan(srcs, NB, H, W, cout, 1, **extra)
    assert [_bm(r) for r in recs] == [(build, 1)], recs
    xs = _inputs(srcs, NB, H, W, 700 + cout)
    w, b = _weights(srcs, cout, 1, 800 + cout)
    out, prev, mask = _launch(ops, [t.cuda() for t in xs], w.cuda(), b.cuda(), srcs, cout, 1, variant, seed=cout)
    _hold(out, xs, w, None if variant == 'nobias' else b, 1, list(range(NB)), recs, f'1x1 {H}x{W} cout {cout} {variant}',
          relu=variant == 'relu', prev=prev, mask=mask)


# ------------------------------------------------------------------ nontemporal stores above 192 MB of output
@pytest.mark.parametrize('ks,build,mp', [(1, P1_64, 1), (3, B64, 2)])
def test_nontemporal_path_gives_the_bits_of_two_halves(ops, ks, build, mp):
    # 64 couts x 56 x 56 x 251 images = 201.5 MB; 8 input channels: the time is the store
    srcs, cout, H, W, NB = [8], 64, 56, 56, 251
    rec, = _plan(srcs, NB, H, W, cout, ks)
    assert _bm(rec) == (build, mp) and rec['nontemporal'] == 1
    halves = [(0, 126), (126, NB)]
    for lo, hi in halves:
        r, = _plan(srcs, hi - lo, H, W, cout, ks)
        assert _bm(r) == (build, mp) and r['nontemporal'] == 0
    x = torch.randn(NB, 8, H, W, generator=_g(900 + ks))
    w, b = _weights(srcs, cout, ks, 910 + ks)
    xd, wq, bd = x.cuda(), ops.pack_conv_weight(w.cuda()), b.cuda()
    buf = torch.full((2 * GUARD + NB * cout * H * W,), CANARY, device='cuda')
    out = buf[GUARD:-GUARD].view(NB, cout, H, W)
    ops.conv2d(xd, wq, bd, cout, ks, out=out)
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())
    for lo, hi in halves:
        assert torch.equal(out[lo:hi], ops.conv2d(xd[lo:hi].contiguous(), wq, bd, cout, ks))
    idx = [0, 1, 125, 126, NB - 2, NB - 1]
    _hold(out, [x], w, b, ks, idx, [rec], f'nontemporal {ks}x{ks}')


# ------------------------------------------------------------------ refusals
def _nb_for(srcs, H, W, cout, build):
    """The smallest batch whose plan is `build` (3x3, Cout > 64: the 128 x 128 build needs more than ~1.45 tiles per CU)."""
    for NB in list(range(2, 40)) + list(range(40, 4000, 10)):
        recs = _plan(srcs, NB, H, W, cout, 3)
        if _bm(recs[0])[0] == build and len(recs) == 1:
            return NB
    raise AssertionError('no batch size reaches the build')


@pytest.mark.parametrize('cout,build', [(72, B32), (72, B128), (36, BTAIL), (64, B64), (32, B32C)], ids=lambda v: NAMES.get(v, str(v)))
def test_maps_168_wide_run_and_169_wide_are_refused(ops, cout, build):
    from dynamask_amd import ops as o
    srcs, H = [12], 1
    NB = _nb_for(srcs, H, 168, cout, build)
    recs = _plan(srcs, NB, H, 168, cout, 3)
    assert [_bm(r) for r in recs] == [(build, 4)]
    xs = _inputs(srcs, NB, H, 168, 1200 + cout)
    w, b = _weights(srcs, cout, 3, 1300 + cout)
    out, _, _ = _launch(ops, [t.cuda() for t in xs], w.cuda(), b.cuda(), srcs, cout, 3)
    _hold(out, xs, w, b, 3, _images(NB, recs, 168, sample=6), recs, f'168 wide, {NAMES[build]}')
    rc, none = o.conv2d_plan_raw(srcs, NB, H, 169, cout, 3)
    assert (rc, none) == (-3, [])
    xs = _inputs(srcs, NB, H, 169, 1200 + cout)
    _launch(ops, [t.cuda() for t in xs], w.cuda(), b.cuda(), srcs, cout, 3, expect_error=-3)


def test_3x3_on_1x1_maps(ops):
    """The 128-pixel tiles cannot stage 128 images of 3 x 3 padded positions (1152 > 1024), the 32-pixel tile can: Cout > 64
    runs the 128 x 32 build whatever NB (it used to be refused from ~1.45 tiles per CU on), Cout <= 64 is refused."""
    srcs, cout = [12], 96
    big = 128 * (3 * CUS) + 77                  # three tiles of 128 pixels per CU: far into what took the 128 x 128 build
    xs = _inputs(srcs, big, 1, 1, 1400)
    w, b = _weights(srcs, cout, 3, 1410)
    outs = {}
    for NB in (big, 3, 200):
        recs = _plan(srcs, NB, 1, 1, cout, 3)
        assert [_bm(r) for r in recs] == [(B32, 2)], recs
        out, _, _ = _launch(ops, [t[:NB].cuda() for t in xs], w.cuda(), b.cuda(), srcs, cout, 3)
        _hold(out, xs, w, b, 3, _images(NB, recs, 1, sample=64), recs, f'3x3 on 1x1 maps, NB {NB}')
        outs[NB] = out
        assert torch.equal(out, outs[big][:NB])
    for c in (64, 36, 32):
        w, b = _weights(srcs, c, 3, 1420 + c)
        _launch(ops, [t[:5].cuda() for t in xs], w.cuda(), b.cuda(), srcs, c, 3, expect_error=-3)


def test_flag_bit_2_is_refused(ops):
    """include/dynamask_hip.h: any flag outside bits 0, 1, 3, 4 is DM_ERR_INVALID_ARG -- bit 2 (the launcher's own
    nontemporal bit) used to be accepted and dropped."""
    from dynamask_amd._lib import lib
    x = torch.randn(2, 8, 14, 14, device='cuda')
    w = torch.randn(16, 8, 1, 1, device='cuda')
    wq = ops.pack_conv_weight(w)
    out = torch.full((2, 16, 14, 14), CANARY, device='cuda')
    ones = torch.ones_like(out)
    vp = ctypes.c_void_p
    for entry, extra in (('dm_conv2d_fwd', ()), ('dm_conv2d_fwd_ws', (None, 0)), ('dm_conv2d_fwd_masked', (vp(ones.data_ptr()),))):
        for flags, want in ((4, -1), (5, -1), (32, -1), (1, 0)):
            rc = getattr(lib(), entry)((vp * 1)(x.data_ptr()), (ctypes.c_int * 1)(8), None, 1, 2, 14, 14, vp(wq.data_ptr()), None, 16, 1,
                                       flags, vp(out.data_ptr()), 16, 0, *extra, None)
            torch.cuda.synchronize()
            assert rc == want, (entry, flags)
            if want:
                assert bool((out == CANARY).all())
            else:
                assert_close_via_f64(out.cpu(), F.conv2d(x.cpu(), w.cpu()).relu(), F.conv2d(x.cpu().double(), w.cpu().double()).relu(),
                                     f'{entry} flags 1')
                out.fill_(CANARY)


# ------------------------------------------------------------------ the workspace path: a K split on the device
@pytest.mark.parametrize('srcs,cout,H,W,NB,ks,build,mp', [([128], 72, 14, 14, 16, 3, B128, 1), ([96, 30, 2], 130, 28, 28, 2, 3, B128, 2),
                                                         ([128], 36, 14, 14, 5, 3, BTAIL, 1)])
def test_split_k_launch_against_float64(ops, srcs, cout, H, W, NB, ks, build, mp):
    from dynamask_amd._lib import lib
    nws = int(lib().dm_conv2d_splitk_floats(NB, H, W, cout, ks))
    assert nws > 0
    recs = _plan(srcs, NB, H, W, cout, ks, workspace_floats=nws)
    assert [_bm(r) for r in recs] == [(build, mp)] and recs[0]['ksplit'] >= 2 and recs[0]['grid_y'] == recs[0]['ksplit'], recs
    assert recs[0]['ksplit'] * NB * cout * H * W <= nws
    xs = _inputs(srcs, NB, H, W, 1500 + cout)
    w, b = _weights(srcs, cout, ks, 1510 + cout)
    with ops.splitk_scope():
        assert ops.CONV_SPLITK[0]
        out, _, _ = _launch(ops, [t.cuda() for t in xs], w.cuda(), b.cuda(), srcs, cout, ks, 'relu')
    _hold(out, xs, w, b, ks, list(range(NB)), recs, f'split-K x{recs[0]["ksplit"]} {H}x{W} cout {cout}', relu=True)


# ------------------------------------------------------------------ coverage
def _all_plans():
    plans = []
    for fam, cat in WIDE_CASES:
        f = FAMS[fam]
        plans += _plan(f['srcs'], _pick(f, cat), f['H'], f['W'], f['cout'], 3)
    for (H, W), _, NB, srcs, cout, _, variant in NARROW_CASES:
        plans += _plan(srcs, NB, H, W, cout, 3, accumulate=variant == 'accumulate')
    for cout, (H, W), srcs in P1_WIDE:
        for NB in _p1_nbs(cout, H, W):
            plans += _plan(srcs, NB, H, W, cout, 1)
    for cout, _, (H, W), srcs, _ in P1_NARROW:
        plans += _plan(srcs, _p1_narrow_nb(H, W), H, W, cout, 1)
    plans += _plan([12], 3, 1, 1, 96, 3)
    plans += _plan([8], 251, 56, 56, 64, 3) + _plan([8], 251, 56, 56, 64, 1)
    return plans


def test_every_build_is_reached():
    """The union of the plans of the sweep above is TABLE: no (build, MAXPOS) pair of the exact launcher is unreached, and no
    case fell outside the table.  On a 256-CU device every category of workgroup counts must have had a case."""
    reached = {_bm(r) for r in _all_plans()}
    assert reached == TABLE, (sorted(TABLE - reached), sorted(reached - TABLE))
    have = {cat for _, cat in WIDE_CASES}
    if CUS == 256:
        assert have == set(CATS)
        for fam in FAMS:
            missing = [c for c in CATS if (fam, c) not in WIDE_CASES]
            assert missing in ([], ['round1']), (fam, missing)        # (exactly one round needs a batch that ends on the tile edge)
    print('\nbuild, MAXPOS: largest |product - f64| / the fp32 reference\'s own error')
    for b, mp in sorted(TABLE):
        e = ERRS.get((b, mp))
        print(f'  {NAMES[b]:<16} MAXPOS {mp}: ' + (f'{e[0]:.3g} / {e[1]:.3g}' if e else 'not run in this session'))
