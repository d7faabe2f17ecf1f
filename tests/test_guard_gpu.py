"""Memory-safety net: every device tensor the package allocates while these tests run --
outputs, scratch, intermediates, and the inputs the tests hand over -- sits between two guard bands of signalling
patterns.  After each pass the bands must be bit-for-bit intact (a kernel stored one past the end, or in front of the
start, of a buffer otherwise) and every result finite (float bands are NaN: an out-of-range READ that reaches a result
poisons it).  Shapes are the odd ones of tools/stress.py: RoI counts 1 / 7 / 129 / 513 on 333x500 ... 2048x1024
pyramids -- magic-number divisions, LDS band staging and the "last round" second launches all see ragged edges."""
import pytest
import torch

import golden_inputs as gi
from guard_arena import Arena, guarded, _put, _finite  # noqa: F401  (the arena lives in guard_arena.py, shared with the surface passes)

pytestmark = pytest.mark.gpu


def _full_head():
    from dynamask_amd import registry, roi_head, losses, mask_heads, roi_extractors, bbox_heads, synth  # noqa: F401
    from dynamask_amd.registry import ConfigDict
    cfg = dict(type='DynaMaskRoIHead',
               bbox_roi_extractor=dict(type='SingleRoIExtractor', **gi.BBOX_ROI_EXTRACTOR_CFG),
               bbox_head=dict(type='Shared2FCBBoxHead', **gi.BBOX_HEAD_CFG),
               mask_roi_extractor=dict(type='SingleRoIExtractor', **gi.MASK_ROI_EXTRACTOR_CFG),
               mask_head=dict(type='DynaMaskHead', **gi.MASK_HEAD_CFG), test_cfg=ConfigDict(**gi.RCNN_TEST_CFG))
    m = registry.build_head(cfg)
    m.load_state_dict({**synth.init_dynamask_head_state(seed=5, test_mode=True), **synth.init_mask_pre_state(seed=6),
                       **synth.init_bbox_head_state(seed=8)}, strict=True)
    return m.cuda()


def test_arena_catches_a_store_past_the_end(monkeypatch):
    """The net itself: a deliberate one-past-the-end store must be reported."""
    with guarded(monkeypatch) as arena:
        t = torch.empty((5, 3), device='cuda')
        assert arena.count == 1 and t.is_contiguous() and t.data_ptr() % 256 == 0
        arena.check()
        t.view(-1).as_strided((16,), (1,))[15] = 1.0          # element 15 of a 15-element buffer
        with pytest.raises(AssertionError, match='guard bands overwritten'):
            arena.check()


def test_launch_log_reports_a_store_outside_the_arena(monkeypatch):
    """The net itself: an ``out=`` from the un-patched factory is a store pointer outside every arena block."""
    from guard_arena import LaunchLog
    from dynamask_amd import hazard, ops
    name = 'dm_maxpool3x3_s2_fwd'
    arg = hazard.parse_header()[name].index('out')
    with guarded(monkeypatch) as arena, LaunchLog(arena) as log:
        x = _put(arena, torch.randn(1, 2, 5, 7, generator=torch.Generator().manual_seed(1)))
        inside = ops.maxpool3x3_s2(x)
        assert log.launches == {name: 1} and log.reached_guarded() == {name} and log.unguarded_stores() == set()
        assert log.stores == {(name, arg): [1, 0]} and log.reads == {(name, 0): [1, 0]}
        out = arena._empty((1, 2, 3, 4), dtype=torch.float32, device='cuda')           # torch.empty as it was
        assert ops.maxpool3x3_s2(x, out=out) is out
        assert log.launches == {name: 2} and log.guarded_launches == {name: 1}
        assert log.unguarded_stores() == {(name, arg)} and log.stores == {(name, arg): [1, 1]}
        assert torch.equal(out, inside)
        arena.check()
    from dynamask_amd import _lib
    assert _lib.lib() is not None and not hasattr(_lib.lib(), '_log'), 'the library proxy was not taken off again'


def test_arena_poisons_a_read_that_reaches_into_a_band(monkeypatch):
    """The net itself: a read one element behind the end, or in front of the start, of a buffer makes the result
    non-finite (float bands are NaN).  A torch-level ``as_strided`` inside the arena's own raw allocation."""
    with guarded(monkeypatch) as arena:
        t = torch.ones((5, 3), device='cuda')
        assert _finite([t.sum(), t])
        behind = t.as_strided((16,), (1,), t.storage_offset())               # elements 0 .. 15 of a 15-element buffer
        before = t.as_strided((15,), (1,), t.storage_offset() - 1)           # element -1 .. 13
        assert not _finite([behind.sum()]) and not _finite([before.sum()])
        assert _finite([t.as_strided((15,), (1,), t.storage_offset()).sum()])
        ints = torch.zeros((4,), dtype=torch.int32, device='cuda')            # integer bands: the NaN pattern read as float
        assert not _finite([ints.as_strided((5,), (1,), ints.storage_offset()).view(torch.float32)])
        arena.check()                                                        # reading breaks no band


@pytest.mark.parametrize('H,W', [(333, 500), (608, 1024), (800, 1333), (1024, 2048)])
def test_inference_surface_keeps_its_guard_bands(monkeypatch, H, W):
    """tools/stress.py as a test: mask head (all exits), per-RoI early exit with the selector, the whole
    simple_test (bbox branch, NMS, masks, device RLE) at RoI counts 1 / 7 / 129 / 513."""
    from dynamask_amd import synth
    m = _full_head().eval()
    with guarded(monkeypatch) as arena:
        feats = [_put(arena, f) for f in synth.make_fpn(1, H, W, 256, seed=H)]
        for N in (1, 7, 129, 513):
            rois = _put(arena, synth.make_rois(1, N, H, W, seed=N))
            labels = _put(arena, synth.make_labels(N, seed=N + 1))
            with torch.no_grad():
                r = m._mask_forward(feats, rois, labels)
                assert _finite(r['stage_instance_preds'] + r['stage_detail_preds']), (H, W, N)
                d = m.dynamic_mask_logits(feats, rois[:, 1:].contiguous(), labels)
                assert _finite(d['preds']), (H, W, N)
                # the fixed 28x28 exit and exits spread over the four resolutions: the logits-of-the-upsampled-stage kernel
                r1 = m._mask_forward(feats, rois, labels, last_stage=1)
                assert _finite(r1['stage_instance_preds']), (H, W, N)
                d2 = m.dynamic_mask_logits(feats, rois[:, 1:].contiguous(), labels, exits=(torch.arange(N) * 7 + 3) % 4)
                assert _finite(d2['preds']), (H, W, N)
                metas = [dict(img_shape=(H, W, 3), ori_shape=(H, W, 3), scale_factor=1.0)]
                bb, sg = m.simple_test(feats, [rois[:, 1:].contiguous()], metas, rescale=False, encode=True)
                assert sum(len(b) for b in bb) == sum(len(s) for s in sg)
            n_blocks = arena.check()
        print(f'{H}x{W}: {n_blocks} guarded device buffers, all bands intact')


@pytest.mark.parametrize('H,W,per', [(333, 500, 7), (800, 1333, 129), (608, 1024, 37)])
def test_training_step_keeps_its_guard_bands(monkeypatch, H, W, per):
    """One training step of the mask path (forward, loss, hand-sequenced backward incl. the DCN / point-sample / RoIAlign
    adjoints, fused SGD) at odd RoI counts, default and deterministic accumulation."""
    from dynamask_amd import ops, synth
    from dynamask_amd.dist import FlatParamGroup, mask_path_parameters
    B = 2
    for det in (False, True):
        monkeypatch.setattr(ops, 'DETERMINISTIC', [det])
        m = _full_head().train()
        with guarded(monkeypatch) as arena:
            feats = [_put(arena, f).requires_grad_(True) for f in synth.make_fpn(B, H, W, 256, seed=H + 1)]
            rois = _put(arena, synth.make_rois(B, per, H, W, seed=per))
            labels = _put(arena, synth.make_labels(B * per, seed=per + 1))
            targets = [_put(arena, t) for t in synth.make_targets(B * per, seed=per + 2)]
            noise = _put(arena, synth.make_gumbel_noise(B * per, seed=per + 3))
            grp = FlatParamGroup(mask_path_parameters(m))
            grp.zero_grad()
            res = m._mask_forward_train(feats, rois, labels, targets, noise=noise)
            res['loss_mask']['loss_masks'].backward()
            grp.sgd_step(lr=0.02, momentum=0.9, weight_decay=1e-4)
            assert _finite([res['loss_mask']['loss_masks'].detach(), grp.flat_grad, grp.flat_param] + [f.grad for f in feats[:4]])
            n_blocks = arena.check()
        print(f'{H}x{W}, 2 x {per} RoIs, deterministic={det}: {n_blocks} guarded device buffers, all bands intact')
