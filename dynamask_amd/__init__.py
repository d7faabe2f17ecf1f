"""dynamask_amd -- MI355X-native (gfx950) DynaMask dynamic mask-head hot path.

Layout:
  csrc/                 HIP kernels + the C ABI (include/dynamask_hip.h)
  _lib.py, ops.py       ctypes binding of libdynamask_hip.so over torch device memory
  registry.py           mmdet-style DETECTORS / BACKBONES / HEADS / NECKS / ROI_EXTRACTORS / LOSSES registries + Config
  layers.py             the parameter holders and weight caches every module below is made of (imports none of them)
  postprocess.py        host-side result code: NMS, mask paste, per-class result lists (imports none of them)
  backbones.py          ResNet, ResNeXt, Res2Net: the image -> the stages the neck reads
  necks.py              FPN, FPN_CARAFE: the backbone's stages -> the maps the RPN and the RoI heads read
  dense_heads.py        RPNHead: the maps -> the proposals (simple_test_rpn, aug_test_rpn); FCOSHead: the maps -> detections
  roi_extractors.py, mask_heads.py, losses.py, roi_head.py
                        host-side mirror of the reference's plugin classes
  detectors.py          MaskRCNN and its siblings, FCOS: decoded images -> results (above all of the modules before it);
                        the image pre-processing in front of the backbone, load_checkpoint
  synth.py              synthetic workload
  dist.py               RCCL gradient all-reduce of the mask-head parameters

There is no CPU or eager-PyTorch fallback: every operator raises if
libdynamask_hip.so is missing or its input is not on a HIP device.
"""
__version__ = '0.1.0'

from .precision import conv_precision, get_conv_precision, set_conv_precision  # noqa: E402,F401


def __getattr__(name):          # NECKS, build_neck, FPN, FPN_CARAFE, BACKBONES, build_backbone, ResNet, ResNeXt, Res2Net, DETECTORS, build_detector: resolved on first use (necks.py imports the operator bindings)
    if name in ('NECKS', 'build_neck'):
        from . import necks, registry  # noqa: F401  (necks registers FPN and FPN_CARAFE)
        return getattr(registry, name)
    if name in ('FPN', 'FPN_CARAFE'):
        from . import necks
        return getattr(necks, name)
    if name in ('BACKBONES', 'build_backbone'):
        from . import backbones, registry  # noqa: F401  (backbones registers ResNet, ResNeXt and Res2Net)
        return getattr(registry, name)
    if name in ('ResNet', 'ResNeXt', 'Res2Net'):
        from . import backbones
        return getattr(backbones, name)
    if name in ('FCOS', 'SingleStageDetector'):
        from . import detectors
        return getattr(detectors, name)
    if name == 'FCOSHead':
        from . import dense_heads
        return dense_heads.FCOSHead
    if name in ('DETECTORS', 'build_detector'):
        from . import detectors, registry  # noqa: F401  (detectors registers MaskRCNN and its siblings)
        return getattr(registry, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
