"""NaN and Inf activations through the forward kernels: the case table and the helpers of tests/test_nonfinite_cpu.py (the
references alone: every case can show a failure) and tests/test_nonfinite_gpu.py (the kernels against them).

The rule ("Non-finite activations"): a NaN or Inf activation leaves every forward kernel as it would leave
torch's operator.  ``plant`` writes four specials into a seeded O(1) tensor -- a lone NaN, a lone +Inf, a lone -Inf, and
a +Inf / -Inf pair that meets in one output's reduction, so that a NaN is born inside the accumulation -- each in an image
of its own and at least two pixels from every border: no padding tap and no void tap of a gather lands on a special (those
are another topic: a zero weight times the clamped pixel it reads).  ``assert_same_nonfinite`` holds the NaN, +Inf and
-Inf patterns to the float64 reference exactly and the finite rest to the project's gate.

One CASES entry per kernel path: ``build()`` -> the CPU inputs (a dict), ``ref(inp)`` -> (fp32, float64) reference made of
torch's own operators, ``run(ops, dev)`` -> the launch on the inputs moved to the GPU, ``plan(ops, inp)`` -> asserts on the
launcher's own plan that the call takes the path the case is named for (None: the entry point has one path or reports
none).  ``can_inf``: whether the operation can return a +Inf for these inputs (the CPU test then asks for one).  Cases with
many images compare the planted ones and the last (``run`` and ``ref`` select the same rows)."""
import functools

import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

NAN, INF = float('nan'), float('inf')


def gen(seed):
    return torch.Generator().manual_seed(seed)


def plant(x, meet='channels', c=0):
    """Writes the four specials into x [N >= 4, C, ...] in place and returns it: NaN in image 0, +Inf in image 1, -Inf in
    image 2 (all in channel ``c``), and in image 3 a +Inf with a -Inf in the next channel at the same position
    (``meet='channels'``: they meet in every reduction over the channels) or at the next position of the same channel
    (``meet='pixels'``: they meet in one 3x3 window / one interpolation / one group).  On maps (4-D) every position is at
    least two pixels from every border."""
    N, C = x.shape[:2]
    sp = tuple(x.shape[2:])
    assert N >= 4 and 0 <= c and c + (meet == 'channels') < C
    if len(sp) == 2:
        H, W = sp
        assert H >= 5 and W >= 6, 'no room for a two-pixel margin'
        pos, nxt = [(2, 2), (H - 3, W - 3), (2, W - 3), (H - 3, 2)], (H - 3, 3)
    elif len(sp) == 1:
        P = sp[0]
        assert P >= 8
        pos, nxt = [(P // 5,), (2 * P // 5,), (3 * P // 5,), (4 * P // 5,)], (4 * P // 5 + 1,)
    else:
        assert not sp and meet == 'channels'
        pos, nxt = [()] * 4, None
    x[(0, c) + pos[0]] = NAN
    x[(1, c) + pos[1]] = INF
    x[(2, c) + pos[2]] = -INF
    x[(3, c) + pos[3]] = INF
    if meet == 'channels':
        x[(3, c + 1) + pos[3]] = -INF
    else:
        x[(3, c) + nxt] = -INF
    return x


def classes(t):
    """(isnan, == +inf, == -inf) of a tensor, on the CPU."""
    t = t.detach().cpu()
    return torch.isnan(t), t == INF, t == -INF


def assert_same_nonfinite(got, ref32, ref64, name):
    """isnan(got) == isnan(ref64), (got == +inf) == (ref64 == +inf), the same for -inf; then every non-finite position
    is replaced by 0 in all three tensors and they go through tolerances.assert_close_via_f64 at its default rel."""
    got, ref32, ref64 = got.detach().cpu(), ref32.detach().cpu(), ref64.detach().cpu()
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref64.shape)
    diff = {k: int((g != r).sum()) for k, g, r in zip(('NaN', '+Inf', '-Inf'), classes(got), classes(ref64))}
    counts = {k: (int(g.sum()), int(r.sum())) for k, g, r in zip(('NaN', '+Inf', '-Inf'), classes(got), classes(ref64))}
    assert not any(diff.values()), (f'{name}: positions whose class differs from the float64 reference: {diff} '
                                    f'(count here, count in the reference: {counts})')
    bad = ~torch.isfinite(ref64)
    z = [torch.where(bad, torch.zeros((), dtype=t.dtype), t) for t in (got, ref32, ref64)]
    return assert_close_via_f64(z[0], z[1], z[2], name)


class Case:
    def __init__(self, id, build, ref, run, plan=None, can_inf=True):
        self.id, self._build, self._ref, self.run, self.plan, self.can_inf = id, build, ref, run, plan, can_inf
        self._inp = self._refs = None

    def inputs(self):
        if self._inp is None:
            self._inp = self._build()
        return self._inp

    def refs(self):
        """(ref32, ref64), computed once and shared by the CPU and the GPU test."""
        if self._refs is None:
            self._refs = tuple(t.detach() for t in self._ref(self.inputs()))
        return self._refs

    def __repr__(self):
        return self.id


def to_dev(inp):
    mv = lambda v: v.cuda() if isinstance(v, torch.Tensor) else [mv(e) for e in v] if isinstance(v, (list, tuple)) else v  # noqa: E731
    return {k: mv(v) for k, v in inp.items()}


def _both(fn):
    """ref(inp) from fn(inp, dtype)."""
    def ref(inp):
        return fn(inp, torch.float32), fn(inp, torch.float64)
    return ref


# ------------------------------------------------------------------------------------------ conv2d and its relatives
KEYS = ('KS', 'WGM', 'WGN', 'WM', 'WN', 'CK', 'TAIL')
B64, BTAIL = (3, 1, 4, 2, 1, 8, 0), (3, 1, 4, 1, 1, 8, 4)          # (the builds of tests/test_conv_builds_gpu.py)
P1_64, P1_32 = (1, 2, 2, 1, 2, 16, 0), (1, 1, 4, 1, 1, 32, 0)


def _conv_inputs(srcs, cout, ks, NB, H, W, seed, extra=()):
    def build():
        cin = sum(srcs)
        xs = [torch.randn(NB, c, H, W, generator=gen(seed + i)) for i, c in enumerate(srcs)]
        plant(xs[0], 'channels')
        d = dict(xs=xs, w=torch.randn(cout, cin, ks, ks, generator=gen(seed + 10)) / (cin * ks * ks) ** 0.5,
                 b=torch.randn(cout, generator=gen(seed + 11)))
        if 'prev' in extra:
            d['prev'] = torch.randn(NB, cout, H, W, generator=gen(seed + 12))
        if 'addend' in extra:
            d['addend'] = torch.randn(NB, cout, H, W, generator=gen(seed + 13))
        if 'small_addend' in extra:
            d['addend'] = torch.randn(NB, cout, (H + 1) // 2, (W + 1) // 2, generator=gen(seed + 14))
            d['iy'], d['ix'] = (torch.arange(H) // 2).int(), (torch.arange(W) // 2).int()
        return d
    return build


def _conv_ref(ks, where='relu'):
    """where: 'relu' (conv + bias -> ReLU), 'accumulate' (+ prev in front of the ReLU), 'post' (+ addend behind it),
    'up' (+ the gathered addend behind it)."""
    def fn(inp, dt):
        y = F.conv2d(torch.cat(inp['xs'], 1).to(dt), inp['w'].to(dt), inp['b'].to(dt), padding=ks // 2)
        if where == 'accumulate':
            y = y + inp['prev'].to(dt)
        y = F.relu(y)
        if where == 'post':
            y = inp['addend'].to(dt) + y
        if where == 'up':
            y = inp['addend'].to(dt)[:, :, inp['iy'].long()][:, :, :, inp['ix'].long()] + y
        return y
    return _both(fn)


def _bm(rec):
    return tuple(rec[k] for k in KEYS)


def _conv_plan(srcs, cout, ks, build, full=None, post=0, split=False, v4=None, **kw):
    def plan(ops, inp):
        NB, _, H, W = inp['xs'][0].shape
        extra = dict(kw)
        if split:
            from dynamask_amd._lib import lib
            extra['workspace_floats'] = int(lib().dm_conv2d_splitk_floats(NB, H, W, cout, ks))
            assert extra['workspace_floats'] > 0, 'no split-K workspace for this shape: the launch would not split'
        recs = ops.conv2d_plan(srcs, NB, H, W, cout, ks, relu=True, **extra)
        assert len(recs) == 1 and _bm(recs[0]) == build and recs[0]['PREC'] == 0 and recs[0]['POST'] == post, recs
        assert (recs[0]['ksplit'] >= 2) == split, recs
        TM, TN = build[1] * build[3] * 32, build[2] * build[4] * 32
        if full is True:        # the 1x1 builds' "full tiles only" branch: every tile inside the output
            assert ks == 1 and cout % TM == 0 and NB * H * W % TN == 0
        if full is False:       # a ragged last tile in both dimensions
            assert (cout - build[6]) % TM != 0 and NB * H * W % TN != 0
        if split:               # H * W % 4 == 0: the vectorised reduce, else the scalar one
            assert (H * W % 4 == 0) == v4
    return plan


def _wq(ops, dev, srcs):
    return ops.pack_conv_weight(dev['w'], src_channels=srcs)


def _conv_case(id, srcs, cout, ks, NB, H, W, seed, build, **kw):
    full, split, v4 = kw.get('full'), kw.get('split', False), kw.get('v4')
    run = lambda ops, dev: ops.conv2d(dev['xs'], _wq(ops, dev, srcs), dev['b'], cout, ks, relu=True)        # noqa: E731
    if split:
        def run(ops, dev):      # noqa: F811
            with ops.splitk_scope():
                assert ops.CONV_SPLITK[0]
                return ops.conv2d(dev['xs'], _wq(ops, dev, srcs), dev['b'], cout, ks, relu=True)
    return Case(id, _conv_inputs(srcs, cout, ks, NB, H, W, seed), _conv_ref(ks), run,
                _conv_plan(srcs, cout, ks, build, full=full, split=split, v4=v4))


def _accumulate_case():
    srcs, cout, ks = [12], 37, 3
    run = lambda ops, dev: ops.conv2d(dev['xs'], _wq(ops, dev, srcs), dev['b'], cout, ks, relu=True, out=dev['prev'].clone(),  # noqa: E731
                                      accumulate=True)
    return Case('conv2d-3x3-accumulate', _conv_inputs(srcs, cout, ks, 4, 14, 14, 120, ('prev',)), _conv_ref(ks, 'accumulate'), run,
                _conv_plan(srcs, cout, ks, B64, full=False, accumulate=True))


def _post_add_case():
    srcs, cout = [16], 33
    run = lambda ops, dev: ops.conv1x1_post_add(dev['xs'], _wq(ops, dev, srcs), dev['b'], cout, dev['addend'], relu=True)  # noqa: E731
    return Case('conv1x1_post_add', _conv_inputs(srcs, cout, 1, 4, 14, 14, 130, ('addend',)), _conv_ref(1, 'post'), run,
                _conv_plan(srcs, cout, 1, P1_64, post=1, has_addend=True))


def _up_add_case():
    srcs, cout = [16], 33
    run = lambda ops, dev: ops.conv2d_up_add(dev['xs'], _wq(ops, dev, srcs), dev['b'], cout, dev['addend'], dev['iy'], dev['ix'],  # noqa: E731
                                             relu=True)
    return Case('conv2d_up_add', _conv_inputs(srcs, cout, 1, 4, 14, 14, 140, ('small_addend',)), _conv_ref(1, 'up'), run)


def _deconv_case():
    C, cout, NB, H, W = 16, 20, 4, 7, 7

    def build():
        return dict(x=plant(torch.randn(NB, C, H, W, generator=gen(150))), w=torch.randn(C, cout, 2, 2, generator=gen(151)) / (C ** 0.5),
                    b=torch.randn(cout, generator=gen(152)))
    ref = _both(lambda inp, dt: F.relu(F.conv_transpose2d(inp['x'].to(dt), inp['w'].to(dt), inp['b'].to(dt), stride=2)))
    run = lambda ops, dev: ops.deconv2x2(dev['x'], ops.pack_deconv_weight(dev['w']), dev['b'], cout, relu=True)  # noqa: E731
    return Case('deconv2x2', build, ref, run)


def _group_case(ks):
    cin, cout, NB, H, W, k = 16, 37 if ks == 3 else 33, 4, 14, 14, 2

    def build():
        return dict(xs=[plant(torch.randn(NB, cin, H, W, generator=gen(160 + ks + i)), c=i) for i in range(k)],
                    ws=[torch.randn(cout, cin, ks, ks, generator=gen(170 + ks + i)) / (cin * ks * ks) ** 0.5 for i in range(k)],
                    bs=[torch.randn(cout, generator=gen(180 + ks + i)) for i in range(k)])

    def fn(inp, dt):
        return torch.stack([F.relu(F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=ks // 2)) for x, w, b in zip(inp['xs'], inp['ws'], inp['bs'])])

    def run(ops, dev):
        wq = [ops.pack_conv_weight(w) for w in dev['ws']]
        if ks == 3:
            return torch.stack(ops.conv2d_group(dev['xs'], wq, dev['bs'], cout, 3, relu=True, split=False))
        return torch.stack(ops.conv1x1_group(dev['xs'], wq, dev['bs'], [cout] * k, relu=True))

    def plan(ops, inp):
        recs = ops.conv2d_group_plan(k, NB, H, W, cin, cout, ks, relu=True)
        assert len(recs) == k and all(_bm(r) == (B64 if ks == 3 else P1_64) and r['ksplit'] == 1 for r in recs), recs
    return Case('conv2d_group-3x3' if ks == 3 else 'conv1x1_group', build, _both(fn), run, plan if ks == 3 else None)


# ------------------------------------------------------------------------------------------ fc
def _fc_case(id, N, K, M, seed, scratch):
    def build():
        return dict(x=plant(torch.randn(N, K, generator=gen(seed))), w=torch.randn(M, K, generator=gen(seed + 1)) / K ** 0.5,
                    b=torch.randn(M, generator=gen(seed + 2)))
    ref = _both(lambda inp, dt: F.relu(F.linear(inp['x'].to(dt), inp['w'].to(dt), inp['b'].to(dt))))

    def plan(ops, inp):
        from dynamask_amd._lib import lib
        assert (int(lib().dm_fc_scratch_floats(N, K, M)) > 0) == scratch, 'the other form of dm_fc_fwd (single pass / with scratch)'
    return Case(id, build, ref, lambda ops, dev: ops.fc(dev['x'], dev['w'], dev['b'], relu=True), plan)


# ------------------------------------------------------------------------------------------ strided and dilated 3x3
def _s2_case(splits):
    C, cout, NB, H, W = 16, 20, 4, 9, 10

    def build():
        return dict(x=plant(torch.randn(NB, C, H, W, generator=gen(200))), w=torch.randn(cout, C, 3, 3, generator=gen(201)) / (9 * C) ** 0.5,
                    b=torch.randn(cout, generator=gen(202)))
    ref = _both(lambda inp, dt: F.relu(F.conv2d(inp['x'].to(dt), inp['w'].to(dt), inp['b'].to(dt), stride=2, padding=1)))
    run = lambda ops, dev: ops.conv3x3_s2(dev['x'], ops.pack_conv_weight(dev['w']), dev['b'], cout, relu=True, splits=splits)  # noqa: E731

    def plan(ops, inp):
        from dynamask_amd._lib import lib
        assert ops.conv3x3_s2_supported(inp['x'], cout, splits)
        if splits:              # 1: the in-kernel epilogue; > 1: the reduce (0: the library's choice between them)
            assert (int(lib().dm_conv3x3_s2_workspace_floats(NB, C, H, W, cout, splits)) > 0) == (splits > 1)
    return Case(f'conv3x3_s2-splits{splits}', build, ref, run, plan)


def _dil_case(kind):
    C, cout, NB, H, W, dils = 16, 20, 4, 9, 10, (1, 3, 5)

    def build():
        return dict(x=plant(torch.randn(NB, C, H, W, generator=gen(210))),
                    ws=[torch.randn(cout, C, 3, 3, generator=gen(211 + i)) / (9 * C) ** 0.5 for i in range(3)],
                    bs=[torch.randn(cout, generator=gen(215 + i)) for i in range(3)])

    def fn(inp, dt):
        ys = [F.relu(F.conv2d(inp['x'].to(dt), w.to(dt), b.to(dt), padding=d, dilation=d)) for w, b, d in zip(inp['ws'], inp['bs'], dils)]
        return ys[1] if kind == 'dil' else ys[0] + ys[1] + ys[2]

    def run(ops, dev):
        wq = [ops.pack_conv_weight(w) for w in dev['ws']]
        if kind == 'dil':
            return ops.conv3x3_dil(dev['x'], wq[1], dev['bs'][1], cout, dils[1], relu=True)
        return ops.conv3x3_multidil(dev['x'], wq, dev['bs'], cout, list(dils), relu=True, fused=kind == 'fused')

    def plan(ops, inp):
        assert ops.conv3x3_dil_supported(inp['x'], cout, dils[1]) and ops.conv3x3_multidil_supported(inp['x'], cout, list(dils))
    return Case('conv3x3_dil' if kind == 'dil' else f'conv3x3_multidil-{kind}', build, _both(fn), run, plan)


# ------------------------------------------------------------------------------------------ deformable convolution
DG = 2
GENERIC, LDS, C256, BAND = range(4)
# (id, build of the launch, 'plain' / 'split', H, W, Cout, C): maps and channel counts of tests/test_dcn_builds_gpu.py::CASES
DCN_ROUTES = [('generic', (GENERIC, 2, 2, 1, 1), 'plain', 7, 7, 40, 16),
              ('lds', (LDS, 0, 0, 0, 0), 'plain', 14, 14, 72, 16),
              ('c256', (C256, 0, 0, 0, 0), 'plain', 14, 14, 232, 16),
              ('band', (BAND, 2, 1, 4, 0), 'plain', 16, 28, 40, 16),
              ('lds+split', (LDS, 0, 0, 0, 0), 'split', 14, 14, 72, 64),
              ('generic+split-odd', None, 'split', 7, 7, 41, 64)]
DCN_MIN_NB, DCN_MAX_NB = 5, 1500


def _dcn_plan(ops, nb, C, H, W, cout, split):
    from dynamask_amd import _lib
    ws = int(_lib.lib().dm_deform_conv_splitk_floats(nb, C, H, W, cout)) if split else 0
    return ops.deform_conv_plan(nb, C, H, W, cout, DG, relu=True, workspace_floats=ws)


def _dcn_build_of(rec):
    return (rec['kernel'], rec['P0'], rec['P1'], rec['P2'], rec['P3'])


@functools.lru_cache(maxsize=None)
def dcn_find(route):
    """The batch search of tests/test_dcn_builds_gpu.py: the smallest batch (from 5 RoIs on) whose plan is the route; on
    the odd split route also one whose output is no multiple of four floats (the scalar reduce)."""
    from dynamask_amd import ops
    _, build, kind, H, W, cout, C = route
    for nb in range(DCN_MIN_NB, DCN_MAX_NB):
        recs = _dcn_plan(ops, nb, C, H, W, cout, kind == 'split')
        if len(recs) != 1 or (build is not None and _dcn_build_of(recs[0]) != build):
            continue
        if (recs[0]['ksplit'] > 1) != (kind == 'split'):
            continue
        if build is None and nb * cout * H * W % 4 == 0:
            continue
        return nb
    raise AssertionError(f'no batch below {DCN_MAX_NB} takes the DCN route {route[0]} on this device')


def _dcn_inputs(N, C, H, W, cout, seed):
    x = plant(torch.randn(N, C, H, W, generator=gen(seed)))
    off = (torch.rand(N, 18 * DG, H, W, generator=gen(seed + 1)) * 2 - 1) * 0.74          # |offset| < 0.75: only border outputs have void taps
    w = torch.randn(cout, C, 3, 3, generator=gen(seed + 2)) / (9 * C) ** 0.5
    return dict(x=x, off=off, w=w)


def _dcn_ref(sel):
    from oracle import ref_ops

    def fn(inp, dt):
        return F.relu(ref_ops.deform_conv2d(inp['x'][sel].to(dt), inp['off'][sel].to(dt), inp['w'].to(dt), 1, 1, 1, DG))
    return _both(fn)


def _dcn_case(route, nb):
    """``nb``: the batch the route was found at on the 256-CU device (the CPU test builds the inputs without asking the
    library); the plan of the GPU test repeats the search and holds the launch to the route."""
    name, build, kind, H, W, cout, C = route
    sel = [0, 1, 2, 3, nb - 1]

    def plan(ops, inp):
        assert dcn_find(route) == nb, (f'the route {name} starts at {dcn_find(route)} RoIs on this device, the case was written for '
                                       f'{nb}')
        rec, = _dcn_plan(ops, nb, C, H, W, cout, kind == 'split')
        assert (build is None or _dcn_build_of(rec) == build) and (rec['ksplit'] > 1) == (kind == 'split'), rec
        if kind == 'split':
            assert rec['reduce'] == 1 and (nb * cout * H * W % 4 == 0) == (build is not None)

    def run(ops, dev):
        wq = ops.pack_conv_weight(dev['w'])
        if kind == 'split':
            with ops.splitk_scope():
                assert ops.CONV_SPLITK[0]
                return ops.deform_conv(dev['x'], dev['off'], wq, cout, DG, relu=True)[sel]
        return ops.deform_conv(dev['x'], dev['off'], wq, cout, DG, relu=True)[sel]
    return Case(f'deform_conv-{name}', lambda: _dcn_inputs(nb, C, H, W, cout, 300 + len(name)), _dcn_ref(sel), run, plan)


def _tout_case(which):
    """deform_conv_tout: relu(DCN) ('dcn': the kept DCN output) and relu(1x1(relu(DCN))) ('chained')."""
    NB, C, H, W, cout, m2 = 48, 64, 16, 28, 64, 20          # the band build whose waves hold every cout: the only one that chains
    sel = [0, 1, 2, 3, NB - 1]

    def build():
        d = _dcn_inputs(NB, C, H, W, cout, 340)
        d.update(w2=torch.randn(m2, cout, 1, 1, generator=gen(343)) / cout ** 0.5, b2=torch.randn(m2, generator=gen(344)))
        return d

    def fn(inp, dt):
        from oracle import ref_ops
        y = F.relu(ref_ops.deform_conv2d(inp['x'][sel].to(dt), inp['off'][sel].to(dt), inp['w'].to(dt), 1, 1, 1, DG))
        return y if which == 'dcn' else F.relu(F.conv2d(y, inp['w2'].to(dt), inp['b2'].to(dt)))

    def run(ops, dev):
        out2 = torch.zeros(NB, m2, H, W, device='cuda')
        dcn = ops.deform_conv_tout(dev['x'], dev['off'], ops.pack_conv_weight(dev['w']), cout, DG, ops.pack_tout_weight(dev['w2']),
                                   dev['b2'], m2, out2, keep_dcn=True)
        return (dcn if which == 'dcn' else out2)[sel]

    def plan(ops, inp):
        assert ops.deform_conv_tout_supported(inp['x'], cout, m2)
        rec, = ops.deform_conv_plan(NB, C, H, W, cout, DG, m2=m2)
        assert _dcn_build_of(rec)[:3] == (BAND, cout // 32, 1) and rec['ksplit'] == 1, rec
    # (chained: the 1x1 sums the DCN's +Inf rows with weights of both signs -- its outputs there are NaN, none +Inf)
    return Case(f'deform_conv_tout-{which}', build, _both(fn), run, plan, can_inf=which == 'dcn')


# ------------------------------------------------------------------------------------------ the other forward kernels
def _gn_case():
    N, C, G, H, W = 4, 12, 3, 7, 9

    def build():
        return dict(x=plant(torch.randn(N, C, H, W, generator=gen(400)), 'pixels', c=5), g=torch.rand(C, generator=gen(401)) + 0.5,
                    b=torch.randn(C, generator=gen(402)))
    ref = _both(lambda inp, dt: F.relu(F.group_norm(inp['x'].to(dt), G, inp['g'].to(dt), inp['b'].to(dt), 1e-5)))

    def plan(ops, inp):
        assert ops.group_norm_supported(inp['x'], G)
    return Case('group_norm', build, ref, lambda ops, dev: ops.group_norm(dev['x'], dev['g'], dev['b'], G, 1e-5, relu=True), plan,
                can_inf=False)


def _up_case(ac, H, W):
    def build():
        return dict(x=plant(torch.randn(4, 3, H, W, generator=gen(410 + W)), 'pixels', c=1))
    ref = _both(lambda inp, dt: F.relu(F.interpolate(inp['x'].to(dt), scale_factor=2, mode='bilinear', align_corners=ac)))
    return Case(f'upsample2x-ac{int(ac)}-{H}x{W}', build, ref, lambda ops, dev: ops.upsample2x(dev['x'], align_corners=ac, relu=True))


def _cl_up_case():
    N, C, H, W, nc = 4, 8, 7, 8, 5

    def build():
        g = gen(420)
        return dict(x=plant(torch.randn(N, C, H, W, generator=g), 'pixels', c=2), wi=torch.randn(nc, C, generator=g) / C ** 0.5,
                    bi=torch.randn(nc, generator=g), wd=torch.randn(nc, C, generator=g) / C ** 0.5, bd=torch.randn(nc, generator=g),
                    labels=torch.tensor([1, 4, 0, 2]))

    def fn(inp, dt):
        up = F.relu(F.interpolate(inp['x'].to(dt), scale_factor=2, mode='bilinear', align_corners=False))
        ar = torch.arange(N)
        inst = F.conv2d(up, inp['wi'].to(dt)[:, :, None, None], inp['bi'].to(dt))[ar, inp['labels']]
        det = F.conv2d(up, inp['wd'].to(dt)[:, :, None, None], inp['bd'].to(dt))[ar, inp['labels']]
        return torch.stack([inst, det], 1)

    def run(ops, dev):
        assert ops.class_logits_up2x_supported(dev['x'])
        inst, det = ops.class_logits_up2x(dev['x'], dev['wi'], dev['bi'], dev['wd'], dev['bd'], dev['labels'])
        return torch.cat([inst, det], 1)
    return Case('class_logits_up2x', build, _both(fn), run)


def _point_mlp_case(fused):
    n, P, HW, ncl, CT = 4, 64, 196, 6, 336

    def build():
        g = gen(430)
        return dict(x=plant(torch.randn(n, CT, P, generator=g), 'channels', c=3),
                    ws=[torch.randn(256, CT, generator=g) * (2.0 / CT) ** 0.5 for _ in range(3)],
                    bs=[torch.randn(256, generator=g) * 0.1 for _ in range(3)], wl=torch.randn(ncl, CT, generator=g) * 0.05,
                    bl=torch.randn(ncl, generator=g) * 0.1, labels=torch.tensor([2, 0, 5, 3]),
                    idx=torch.stack([torch.sort(torch.randperm(HW, generator=g)[:P]).values for _ in range(n)]).int(),
                    refined=torch.randn(n, 1, HW, generator=g))

    def fn(inp, dt):
        x = inp['x'].to(dt)
        h, coarse = x[:, :256], x[:, 256:]
        for w, b in zip(inp['ws'], inp['bs']):
            h = F.relu(torch.einsum('ok,nkp->nop', w.to(dt), torch.cat([h, coarse], 1)) + b.to(dt)[None, :, None])
        logits = torch.einsum('ok,nkp->nop', inp['wl'].to(dt), torch.cat([h, coarse], 1)) + inp['bl'].to(dt)[None, :, None]
        out = inp['refined'].to(dt).clone()
        out.view(n, HW).scatter_(1, inp['idx'].long(), logits[torch.arange(n), inp['labels']])
        return out

    def run(ops, dev):
        wq = [ops.pack_conv_weight(w[:, :, None, None].contiguous()) for w in dev['ws']]
        return ops.point_mlp_scatter(dev['x'], wq, dev['bs'], dev['wl'], dev['bl'], dev['labels'], dev['idx'], dev['refined'].clone(),
                                     fused=fused)

    def plan(ops, inp):
        assert ops.point_mlp_supported(inp['x'], 3, ncl, HW)
    # (no +Inf: the second layer sums the first's +Inf rows with weights of both signs -- NaN)
    return Case(f'point_mlp_scatter-{"fused" if fused else "unfused"}', build, _both(fn), run, plan, can_inf=False)


def _point_refine_case(form):
    n, C, NC, S, P = 4, 64, 80, 14, 64

    def build():
        g = gen(440)
        return dict(x=plant(torch.randn(n, C + NC, P, generator=g), 'channels', c=3),
                    ws=[torch.randn(C, C + NC, generator=g) * (2.0 / (C + NC)) ** 0.5 for _ in range(3)],
                    bs=[torch.randn(C, generator=g) * 0.1 for _ in range(3)], feat=torch.randn(n, C, S, S, generator=g),
                    idx=torch.stack([torch.randperm(S * S, generator=g)[:P].sort().values for _ in range(n)]).int())

    def fn(inp, dt):
        x = inp['x'].to(dt)
        h, coarse = x[:, :C], x[:, C:]
        for L, (w, b) in enumerate(zip(inp['ws'], inp['bs'])):
            y = torch.einsum('ok,nkp->nop', w.to(dt), torch.cat([h, coarse], 1)) + b.to(dt)[None, :, None]
            h = F.relu(y) if L < 2 else y
        feat = inp['feat'].to(dt).clone()
        feat.view(n, C, -1).scatter_(2, inp['idx'].long()[:, None].expand(-1, C, -1), h)
        return feat

    def run(ops, dev):
        wq = [ops.pack_conv_weight(w.view(C, -1, 1, 1).contiguous()) for w in dev['ws']]
        return ops.point_refine_mlp(dev['x'], C, wq, dev['bs'], dev['idx'], dev['feat'].clone(), form=form)

    def plan(ops, inp):
        assert ops.point_refine_mlp_supported(n, C, NC, P, 2, S * S)
    return Case(f'point_refine_mlp-{form}', build, _both(fn), run, plan, can_inf=False)      # (as the point MLP: the next layer mixes the Inf rows)


def pool_case(H, W):
    """bn_relu_maxpool with finite statistics passed in (the eval form): max_pool2d(relu(affine))."""
    N, C = 4, 3

    def build():
        g = gen(450 + W)
        return dict(x=plant(torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3, 'pixels', c=1), mean=torch.randn(C, generator=g) * 0.2,
                    var=torch.rand(C, generator=g) + 0.5, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.2)
    ref = _both(lambda inp, dt: pool_ref(inp, dt)[0])
    run = lambda ops, dev: ops.bn_relu_maxpool(dev['x'], dev['mean'], dev['var'], dev['gamma'], dev['beta'], 1e-5)  # noqa: E731
    return Case(f'bn_relu_maxpool-{H}x{W}', build, ref, run)


def pool_ref(inp, dt):
    """(max_pool2d(relu(batch_norm(eval))), its indices) in ``dt``."""
    z = F.relu(F.batch_norm(inp['x'].to(dt), inp['mean'].to(dt), inp['var'].to(dt), inp['gamma'].to(dt), inp['beta'].to(dt), False, 0.1, 1e-5))
    return F.max_pool2d(z, 3, 2, 1, return_indices=True)


POOL_MAPS = ((12, 20), (7, 9))          # even width: the rows kernel; 7 x 9: the generic one

# the batch at which tests/test_dcn_builds_gpu.py's search finds each route on the 256-CU MI355X (dcn_find; held by the plan)
DCN_NB = {'generic': 5, 'lds': 76, 'c256': 38, 'band': 48, 'lds+split': 5, 'generic+split-odd': 5}

CASES = [
    _conv_case('conv2d-3x3-store_all-ragged', [12], 37, 3, 4, 14, 14, 100, B64, full=False),
    _conv_case('conv2d-1x1-store_all-ragged', [16], 33, 1, 4, 14, 14, 101, P1_64, full=False),
    _conv_case('conv2d-1x1-full-tiles', [16], 32, 1, 4, 8, 8, 102, P1_32, full=True),
    _accumulate_case(),
    _conv_case('conv2d-3x3-tail-36', [12], 36, 3, 4, 14, 14, 103, BTAIL),
    _post_add_case(),
    _up_add_case(),
    _deconv_case(),
    _conv_case('conv2d-3x3-splitk-vector-reduce', [128], 36, 3, 5, 14, 14, 104, BTAIL, split=True, v4=True),
    _conv_case('conv2d-3x3-splitk-scalar-reduce', [128], 36, 3, 5, 7, 9, 105, BTAIL, split=True, v4=False),
    _group_case(3),
    _group_case(1),
    _fc_case('fc-single-pass', 12, 24, 13, 190, False),
    _fc_case('fc-scratch-width-div4', 12, 1024, 16, 191, True),
    _fc_case('fc-scratch-width-odd', 12, 1024, 13, 192, True),
    _s2_case(0),
    _s2_case(1),
    _s2_case(2),
    _dil_case('dil'),
    _dil_case('fused'),
    _dil_case('unfused'),
] + [_dcn_case(r, DCN_NB[r[0]]) for r in DCN_ROUTES] + [
    _tout_case('dcn'),
    _tout_case('chained'),
    _gn_case(),
    _up_case(False, 7, 8), _up_case(True, 7, 8), _up_case(False, 7, 9), _up_case(True, 7, 9),
    _cl_up_case(),
    _point_mlp_case(True), _point_mlp_case(False),
    _point_refine_case('fused'), _point_refine_case('unfused'),
] + [pool_case(H, W) for H, W in POOL_MAPS]
