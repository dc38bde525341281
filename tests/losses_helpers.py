"""Helpers shared by tests/test_losses_cpu.py and tests/test_gpu_losses.py: the zero-padded cross-correlation of the oracle
(``oracle.convops.xcorr_torch``'s arithmetic) for any dtype, its adjoint, the crop mask and the oracle's NS kernels."""
import torch
import torch.nn.functional as F

from oracle import residuals as orr


def D(f, k):
    """zero-padded cross-correlation of [B,*ext] with a 3^nd kernel (the arithmetic of oracle.convops.xcorr_torch)"""
    conv = F.conv3d if k.dim() == 3 else F.conv2d
    return conv(f.unsqueeze(1), k[None, None], padding=1).squeeze(1)


def DT_(g, k):
    """the adjoint: the same star with mirrored taps"""
    return D(g, torch.flip(k, dims=tuple(range(k.dim()))))


def _mask(shape, crop):
    m = torch.zeros(shape, dtype=torch.float64)
    if crop:
        m[(Ellipsis,) + (slice(1, -1),) * (len(shape) - 1)] = 1
    else:
        m[...] = 1
    return m


def _k64(op):
    return op.kernel.detach().double()


def ns_kernels():
    o = orr.Ops2D()
    return _k64(o.D_t), _k64(o.D_x), _k64(o.D_y), _k64(o.D_xx_yy)


