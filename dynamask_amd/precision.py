"""Arithmetic of the implicit-GEMM convolutions (csrc/conv_igemm.hip) in inference calls.

``'fp32'`` (the default): the exact fp32 kernel, the parity build.
``'bf16x3'``: each fp32 operand is split into three bf16 planes (x = hi + mid + lo) and a product is the six largest
cross terms on the bf16 matrix cores, accumulated in fp32 -- an error at fp32 level, not the exact fp32 chain.

The mode plays the role ``torch.set_float32_matmul_precision`` plays for matmuls, for this library's convolutions only
(it does not follow torch's setting).  It applies to calls made while ``torch.is_grad_enabled()`` is False; training,
backward, MaskPre and the selector, the DCN kernels and ``fc_gemm`` always run exact fp32, and ops.py routes each
shape to the kernel that is faster for it (ops.BF16X3_ROUTES).  ``DM_CONV_PRECISION`` sets the mode at import."""
import os

PRECISIONS = ('fp32', 'bf16x3')


def checked(p):
    if p not in PRECISIONS:
        raise ValueError(f'unknown convolution precision {p!r}: expected one of {PRECISIONS}')
    return p


_MODE = [checked(os.environ.get('DM_CONV_PRECISION', 'fp32'))]


def set_conv_precision(p):
    """Select the arithmetic of inference convolutions: ``'fp32'`` (default) or ``'bf16x3'``."""
    _MODE[0] = checked(p)


def get_conv_precision():
    return _MODE[0]


class conv_precision:
    """``with conv_precision('bf16x3'): ...`` -- the mode inside the block, the previous one restored after it."""

    def __init__(self, p):
        self.p = checked(p)
        self.prev = None

    def __enter__(self):
        self.prev = _MODE[0]
        _MODE[0] = self.p
        return self

    def __exit__(self, *exc):
        _MODE[0] = self.prev
        return False
