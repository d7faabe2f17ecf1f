"""Inputs, float references and routes shared by tests/test_mask_pre_gpu.py (and the route names the older MaskPre cases of
tests/test_bwd_gpu.py and tests/test_nonfinite_gpu.py assert).  Everything here runs on the CPU.

The inputs: x is drawn from the multiples of 1/8 in [-4, 4].  BatchNorm -> ReLU is, per channel, a non-decreasing function
of x (gamma > 0), so equal x give bit-equal z = relu(bn(x)) in any arithmetic, and unequal x differ by 1/8 * gamma / std
> 0.02, far more than any rounding: which tap of a window holds the first maximum is a property of x, and fp32 autograd,
fp64 autograd and the kernels must agree on it exactly -- ties included (a few per cent of the windows hold their maximum
in more than one tap).  `reference` asserts that much of the two references before anything is compared with them."""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def inputs(NB, C, H, W, seed=900):
    """x on the 1/8 grid, gamma in [0.5, 1.5], beta ~ 0.2 N(0, 1), grad_out ~ N(0, 1), the running statistics to start from"""
    g = gen(seed + 7 * NB + 13 * C + 17 * H + 19 * W)
    x = torch.randint(-32, 33, (NB, C, H, W), generator=g).float() / 8
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    go = torch.randn(NB, C, *out_hw(H, W), generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return dict(x=x, gamma=gamma, beta=beta, go=go, rm=rm, rv=rv)


def _autograd(inp, dt, momentum):
    x, gamma, beta = (inp[k].to(dt).clone().requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    rm, rv = inp['rm'].to(dt).clone(), inp['rv'].to(dt).clone()
    z = F.relu(F.batch_norm(x, rm, rv, gamma, beta, True, momentum, EPS))
    out, idx = F.max_pool2d(z, 3, 2, 1, return_indices=True)
    out.backward(inp['go'].to(dt))
    flat = x.detach().transpose(0, 1).reshape(x.shape[1], -1)
    return dict(out=out.detach(), idx=idx, grad_x=x.grad, grad_gamma=gamma.grad, grad_beta=beta.grad, mean=flat.mean(1),
                var=flat.var(1, unbiased=False), running_mean=rm, running_var=rv)


def tied_share(x, positive):
    """Of the windows that pass a gradient, the share whose maximum sits in more than one tap (equal x: equal z)."""
    NB, C, H, W = x.shape
    taps = F.unfold(F.pad(x, (1, 1, 1, 1), value=float('-inf')).view(NB * C, 1, H + 2, W + 2), 3, stride=2)      # [NB * C, 9, OH * OW]
    multi = ((taps == taps.max(1, keepdim=True).values).sum(1) > 1).view(positive.shape)
    return float((multi & positive).sum()) / max(int(positive.sum()), 1)


def activation(inp, dt):
    """z = relu(bn(x)) with train-mode statistics, the pooling's input"""
    return F.relu(F.batch_norm(inp['x'].to(dt), None, None, inp['gamma'].to(dt), inp['beta'].to(dt), True, 0.1, EPS))


@functools.lru_cache(maxsize=6)       # (the large cases hold tens of megabytes each; the small shapes several tests share are cheap)
def reference(NB, C, H, W, momentum=0.1):
    """(fp32 autograd, fp64 autograd) of the block on inputs(NB, C, H, W), computed once per shape and shared (read only).
    Asserted of the references alone: equal indices, equal sets of windows that pass a gradient, and on maps of 10 x 6 or
    more a tied share above 1 %."""
    inp = inputs(NB, C, H, W)
    r32, r64 = _autograd(inp, torch.float32, momentum), _autograd(inp, torch.float64, momentum)
    assert torch.equal(r32['idx'], r64['idx']), 'the fp32 and fp64 references pool different taps'
    positive = r64['out'] > 0
    assert torch.equal(r32['out'] > 0, positive), 'the fp32 and fp64 references pass a gradient at different windows'
    share = tied_share(inp['x'], positive)
    if H * W >= 60 and min(H, W) >= 6:
        assert share > 0.01, f'only {share:.2%} of the windows hold a tie: the inputs do not exercise the first-maximum rule'
    r64['tied_share'] = share
    return r32, r64


SUMS = 'pool_sums'


def route(ops, op, NB, C, H, W, **kw):
    """[(kernel name, P0, P1)] of the plan's records"""
    return [(ops.MASK_PRE_KERNELS[r['kernel']], r['P0'], r['P1']) for r in ops.mask_pre_plan(op, NB, C, H, W, **kw)]


def sums_channels(ops):
    """The smallest channel count whose backward takes the sums kernel on this device (64 at 256 compute units)."""
    for c in range(1, 4097):
        if route(ops, 'bwd', 16, c, 12, 20)[0][0] == SUMS:
            return c
    raise AssertionError('no channel count below 4097 takes the sums route on this device')


# the backward's forms by the names the older cases use in their comments and ids: (pooling adjoint, BatchNorm backward)
PLAIN_BN, SPLIT_BN, SUMS_BN = [('bn_bwd', 0, 0)], [('bn_bwd_split', 0, 0), ('bn_bwd_split', 1, 0)], [('bn_bwd_split', 1, 0)]
BWD_FORMS = {
    'sums kernel, 2x2 blocks': [(SUMS, 1, 1)] + SUMS_BN,
    'sums kernel, element form': [(SUMS, 0, 1)] + SUMS_BN,
    'plane in LDS': [('pool_lds', 0, 0)] + PLAIN_BN,
    'plane in LDS + split BatchNorm backward': [('pool_lds', 0, 0)] + SPLIT_BN,
    'atomic scatter': [('pool_scatter', 0, 0)] + PLAIN_BN,
    'atomic scatter + split BatchNorm backward': [('pool_scatter', 0, 0)] + SPLIT_BN,
}
