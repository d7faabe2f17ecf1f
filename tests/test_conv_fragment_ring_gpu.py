"""The K loop of the conv_igemm builds without an A image in LDS (csrc/conv_igemm.hip: a ring of weight-fragment sets that
runs on through the chunks, the next chunk's staging loads unpredicated -- clamped addresses, zeros selected at commit)
held to the bits of builds that keep the LDS image and the predicated staging loads.

Every exact build adds an output's products in the order chunk -> tap -> quad pair -> element, so a row of a 128 x 128
launch must equal the same row of launches small enough for the launcher to take 32-pixel tiles.  Each case asks the
launcher (ops.conv2d_plan) which build every launch takes, so that no build is compared with itself, runs the large launch
at the smallest batch whose plan is one 128 x 128 launch, and also holds it to float64 (tolerances.assert_close_via_f64).

What the ring and the clamped loads could get wrong, and where it would show:
  * chunk counts 1 .. 5 (every residue of a ring of 2, 3 or 4 sets), a single chunk, source changes, ragged chunks;
  * a clamped load reaching an MFMA: every source holds Inf at pixel (0, 0) of every image -- the address a padding
    position and a position past the plane read -- so outside the outputs that see that pixel the rows must still equal the
    small build's (an Inf staged where a zero belongs makes Inf or NaN);
  * a fragment or a staging load past its tensor: packed weights and sources lie at the front of NaN-filled buffers;
  * split-K (a split starts the ring at a later chunk): the workspace launch takes the 128 x 128 build at every batch size
    at which it splits, so no launch of another build adds in its order -- it is held to float64 only;
  * the 1x1 builds take the loop only in a library built with -DDM_CONV_DIRECT_A=3: their cases hold whichever loop the
    library has, POST twin included."""
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

KEYS = ('KS', 'WGM', 'WGN', 'WM', 'WN', 'CK', 'TAIL', 'PREC', 'POST')
B128, B32 = (3, 2, 2, 2, 2, 8, 0, 0, 0), (3, 4, 1, 1, 1, 8, 0, 0, 0)
P128, PSMALL = (1, 2, 2, 2, 2, 16, 0, 0, 0), (1, 4, 1, 1, 1, 32, 0, 0, 0)
GUARD = 1 << 14


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _plan(ops, srcs, NB, H, W, cout, ks, **kw):
    return ops.conv2d_plan(list(srcs), NB, H, W, cout, ks, **kw)


def _builds(ops, *a, **kw):
    return [tuple(r[k] for k in KEYS) for r in _plan(ops, *a, **kw)]


def _smallest_big(ops, srcs, H, W, cout, ks, big, maxpos, most=400, **kw):
    """The smallest batch whose plan is one launch of the build `big` with `maxpos` plane positions per thread."""
    for n in range(1, most + 1):
        recs = _plan(ops, srcs, n, H, W, cout, ks, **kw)
        if len(recs) == 1 and tuple(recs[0][k] for k in KEYS) == big and recs[0]['MAXPOS'] == maxpos and recs[0]['ksplit'] == 1:
            return n
    raise AssertionError(f'no batch of at most {most} takes one launch of {big}, MAXPOS {maxpos}')


def _largest_small(ops, srcs, H, W, cout, ks, small, below, **kw):
    for n in range(below - 1, 0, -1):
        if _builds(ops, srcs, n, H, W, cout, ks, **kw) == [small]:
            return n
    raise AssertionError(f'no batch below {below} takes {small}')


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _guarded(t):
    """t on the device, at the front of a NaN-filled buffer."""
    buf = torch.full((t.numel() + GUARD,), float('nan'), device='cuda')
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf[:t.numel()].view(t.shape)


def _problem(ops, srcs, NB, H, W, cout, ks, seed):
    cin = sum(srcs)
    w = torch.randn(cout, cin, ks, ks, generator=_g(seed)) / (cin * ks * ks) ** 0.5
    b = torch.randn(cout, generator=_g(seed + 1))
    clean = [torch.randn(NB, c, H, W, generator=_g(seed + 2 + i)) for i, c in enumerate(srcs)]
    xs = [t.clone() for t in clean]
    for t, c in zip(xs, clean):
        t[:, :, 0, 0] = float('inf')      # the pixel every clamped load reads
        c[:, :, 0, 0] = 0.                # the reference of the outputs that do not see it
    seen = torch.zeros(H, W, dtype=torch.bool)
    seen[:ks // 2 + 1, :ks // 2 + 1] = True
    wq = ops.pack_conv_weight(w.cuda(), src_channels=list(srcs))
    return dict(w=w, b=b, clean=clean, xs_dev=[_guarded(t) for t in xs], b_dev=b.cuda(), wq=_guarded(wq), unseen=~seen, ks=ks,
                cout=cout)


def _run(ops, p, lo, hi, addend=None, split=False):
    xs = [t[lo:hi].contiguous() for t in p['xs_dev']]      # (the whole batch: the guarded tensor itself)
    if addend is not None:
        return ops.conv1x1_post_add(xs, p['wq'], p['b_dev'], p['cout'], addend[lo:hi].cuda(), relu=True)
    if split:
        with ops.splitk_scope():
            return ops.conv2d(xs, p['wq'], p['b_dev'], p['cout'], p['ks'], relu=True)
    return ops.conv2d(xs, p['wq'], p['b_dev'], p['cout'], p['ks'], relu=True)


def _in_chunks(NB, step, fn):
    return torch.cat([fn(i, min(i + step, NB)) for i in range(0, NB, step)])


def _sample(NB, step, most=8):
    idx = {0, 1, NB - 2, NB - 1} | {i for s in range(step, NB, step) for i in (s - 1, s)}
    return sorted(i for i in idx if 0 <= i < NB)[:most]


def _check_f64(p, out, idx, name, addend=None):
    """The outputs that do not see the poisoned pixel against float64."""
    x = torch.cat([t[idx] for t in p['clean']], 1)
    r32 = F.conv2d(x, p['w'], p['b'], padding=p['ks'] // 2).relu()
    r64 = F.conv2d(x.double(), p['w'].double(), p['b'].double(), padding=p['ks'] // 2).relu()
    if addend is not None:
        r32, r64 = r32 + addend[idx], r64 + addend[idx].double()
    m = p['unseen']
    got = out[idx].cpu()
    assert torch.isfinite(got[:, :, m]).all(), f'{name}: a non-finite output away from the poisoned pixel'
    assert_close_via_f64(got[:, :, m], r32[:, :, m], r64[:, :, m], name)


def _check_bits(p, big, ref, name):
    m = p['unseen'].to(big.device)
    assert torch.equal(big[:, :, m], ref[:, :, m]), f'{name}: rows differ from the 32-pixel build\'s'
    assert torch.equal(torch.isnan(big), torch.isnan(ref)), f'{name}: NaN pattern differs'
    assert torch.equal(torch.isinf(big), torch.isinf(ref)), f'{name}: Inf pattern differs'


def _case(ops, srcs, H, W, cout, ks, big, small, maxpos, seed, post=False):
    pk = dict(relu=True, has_addend=post)
    NB = _smallest_big(ops, srcs, H, W, cout, ks, big, maxpos, **pk)
    step = _largest_small(ops, srcs, H, W, cout, ks, small, NB, **pk)
    p = _problem(ops, srcs, NB, H, W, cout, ks, seed)
    addend = torch.randn(NB, cout, H, W, generator=_g(seed + 9)) if post else None
    ref = _in_chunks(NB, step, lambda lo, hi: _run(ops, p, lo, hi, addend))
    out = _run(ops, p, 0, NB, addend)
    name = f'{ks}x{ks} {tuple(srcs)} -> {cout} @{H} NB {NB}'
    _check_bits(p, out, ref, name)
    _check_f64(p, out, _sample(NB, step), name, addend)
    return NB


# ------------------------------------------------------------------ 3x3
@pytest.mark.parametrize('cin', [8, 16, 24, 32, 40])
def test_3x3_chunk_counts(ops, cin):
    _case(ops, (cin,), 14, 14, 256, 3, B128, B32, 1, seed=100 + cin)


@pytest.mark.parametrize('srcs', [(3,), (12,), (16, 3), (16, 16, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_3x3_sources_130_couts_ragged_pixels(ops, srcs):
    # 130 couts: the second cout tile clamps its rows
    NB = _case(ops, srcs, 14, 14, 130, 3, B128, B32, 1, seed=200 + sum(srcs))
    assert (NB * 196) % 128 != 0, 'the last pixel tile is meant to be ragged'


@pytest.mark.parametrize('H,W,maxpos', [(28, 28, 2), (56, 56, 2), (12, 80, 4)])
def test_3x3_map_sizes(ops, H, W, maxpos):
    # (a 128-pixel tile of a 56 x 56 map is a plane of 8 rows of 58: two positions per thread; four from 72 columns on)
    _case(ops, (16, 3), H, W, 130, 3, B128, B32, maxpos, seed=300 + W)


def test_3x3_split_k_starts_at_a_later_chunk(ops):
    srcs, cout, H, W = (100, 24, 3), 256, 14, 14      # 13 + 3 + 1 chunks (the launcher splits from 13 on): the first source ends ragged
    lib_ws = lambda n: int(ops.lib().dm_conv2d_splitk_floats(n, H, W, cout, 3))
    NB = None
    for n in range(1, 121):
        nws = lib_ws(n)
        recs = _plan(ops, srcs, n, H, W, cout, 3, relu=True, workspace_floats=nws) if nws > 0 else []
        if len(recs) == 1 and tuple(recs[0][k] for k in KEYS) == B128 and recs[0]['ksplit'] >= 2:
            NB = n
            break
    assert NB is not None, 'no batch splits K on the 128 x 128 build'
    # the exemption from the bit comparison, checked: at no batch size does a launch that splits take another build
    for n in range(1, 121):
        nws = lib_ws(n)
        for r in (_plan(ops, srcs, n, H, W, cout, 3, relu=True, workspace_floats=nws) if nws > 0 else []):
            assert r['ksplit'] == 1 or tuple(r[k] for k in KEYS) == B128, f'NB {n}: a split launch of another build -- compare with it'
    assert 0 < recs[0]['kchunks'] < 17
    p = _problem(ops, srcs, NB, H, W, cout, 3, seed=400)
    out = _run(ops, p, 0, NB, split=True)
    _check_f64(p, out, _sample(NB, NB), f'3x3 split-K NB {NB} ksplit {recs[0]["ksplit"]}')
    # the unsplit launch of the same shape adds in another order: equal within the same float64 bound, same Inf / NaN pattern
    plain = _run(ops, p, 0, NB)
    assert torch.equal(torch.isfinite(out), torch.isfinite(plain))


def test_3x3_main_launch_and_last_round(ops):
    srcs, cout, H, W, NB = (16,), 256, 14, 14, 512
    recs = _plan(ops, srcs, NB, H, W, cout, 3, relu=True)
    assert [tuple(r[k] for k in KEYS) for r in recs] == [B128, B32] and recs[1]['q_begin'] > 0
    step = _largest_small(ops, srcs, H, W, cout, 3, B32, 64, relu=True)
    p = _problem(ops, srcs, NB, H, W, cout, 3, seed=500)
    ref = _in_chunks(NB, step, lambda lo, hi: _run(ops, p, lo, hi))
    out = _run(ops, p, 0, NB)
    _check_bits(p, out, ref, '3x3 main + last round')
    _check_f64(p, out, _sample(NB, 128), '3x3 main + last round')


# ------------------------------------------------------------------ 1x1
@pytest.mark.parametrize('post', [False, True], ids=['plain', 'post_add'])
@pytest.mark.parametrize('srcs,cout', [((256,), 256), ((16, 16, 2), 128), ((20,), 130)], ids=['256-256', '16x16x2-128', '20-130'])
def test_1x1(ops, srcs, cout, post):
    big, small = (P128[:8] + (1,), PSMALL[:8] + (1,)) if post else (P128, PSMALL)
    _case(ops, srcs, 14, 14, cout, 1, big, small, 1, seed=600 + sum(srcs) + cout, post=post)
