"""Corner pooling (CornerNet) and the TL / BR pooling blocks of the corner-point-verification head
(mmdet/ops/corner_pool/corner_pool.py:7-177).

`CornerPool(mode)`: running maximum towards one image border -- 'top' pools upwards (out[y] = max over rows >= y),
'bottom' downwards, 'left' / 'right' likewise along x.  The reference's compiled `corner_pool_ext` is dead code on
torch >= 1.5 (it takes the `torch.cummax` branch, :93-102).

On the device the pools run as kernels of the library (lsn_corner_pool_forward / _backward, csrc/pool.hip): a lane walks its
line towards the border, so 'top' and 'left' need no flipped copies, and `pool1(a) + pool2(b)` of the pooling blocks is two
launches, the second adding into the first one's output.  The backward walks the line again with torch.cummax's tie rule
(the latest maximum in scan order wins; the inputs are post-ReLU, so ties are the common case) and sums the gradients of a
run of outputs in scan order before it stores them once: no scatter_add, no fp32 atomics, the same bits on every run.  Host
tensors, other layouts and LSNET_NATIVE_POOL=0 (ops/pool.py) take the flip / cummax statements."""
import torch
import torch.nn as nn

from ..cnn.bricks import ConvModule
from . import pool as _pool
from .backend import get_backend
from .conv import Conv2d
from .group_norm import GroupNorm


class _CornerPoolFn(torch.autograd.Function):
    """pool_a(a), or pool_a(a) + pool_b(b) with the second pool accumulating into the first one's output."""

    @staticmethod
    def forward(ctx, mode_a, a, mode_b, b):
        be = get_backend(a)
        y = be.corner_pool_forward(mode_a, a)
        if b is not None:
            be.corner_pool_forward(mode_b, b, out=y, accumulate=True)
        ctx.modes = (mode_a, mode_b)
        ctx.save_for_backward(*([a] if b is None else [a, b]))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        go = _pool._grad_arg(go)
        be = get_backend(go)
        grads = [be.corner_pool_backward(mode, x, go) if need else None
                 for mode, x, need in zip(ctx.modes, ctx.saved_tensors, (ctx.needs_input_grad[1], ctx.needs_input_grad[3]))]
        return None, grads[0], None, (grads[1] if len(grads) > 1 else None)


def _cummax_pool(x, mode):
    dim, flip = CornerPool.DIM_FLIP[mode]
    if flip:
        x = x.flip(dim)
    out = torch.cummax(x, dim=dim)[0]
    return out.flip(dim) if flip else out


def corner_pool(x, mode):
    if _pool.native_ok(x):
        return _CornerPoolFn.apply(mode, x, None, None)
    _pool._fallback('corner_pool', x, f'{mode}, input {_pool._describe(x)}')
    return _cummax_pool(x, mode)


def corner_pool_sum(a, mode_a, b, mode_b):
    """corner_pool(a, mode_a) + corner_pool(b, mode_b)"""
    if a.shape == b.shape and _pool.native_ok(a, b):
        return _CornerPoolFn.apply(mode_a, a, mode_b, b)
    return corner_pool(a, mode_a) + corner_pool(b, mode_b)


class CornerPool(nn.Module):

    DIM_FLIP = {'bottom': (2, False), 'left': (3, True), 'right': (3, False), 'top': (2, True)}

    def __init__(self, mode):
        super().__init__()
        assert mode in self.DIM_FLIP
        self.mode = mode

    def forward(self, x):
        return corner_pool(x, self.mode)


class CornerPoolPack(nn.Module):
    """Two pooled branches (summed, 3x3 conv, GN) + a 1x1 skip branch (conv, GN) -> ReLU -> ConvModule."""

    def __init__(self, dim, pool1, pool2, conv_cfg=None, norm_cfg=None, first_kernel_size=3, kernel_size=3,
                 corner_dim=128):
        super().__init__()
        k1 = first_kernel_size
        self.p1_conv1 = ConvModule(dim, corner_dim, k1, stride=1, padding=(k1 - 1) // 2, conv_cfg=conv_cfg,
                                   norm_cfg=norm_cfg)
        self.p2_conv1 = ConvModule(dim, corner_dim, k1, stride=1, padding=(k1 - 1) // 2, conv_cfg=conv_cfg,
                                   norm_cfg=norm_cfg)
        self.p_conv1 = Conv2d(corner_dim, dim, 3, padding=1, bias=False)
        self.p_gn1 = GroupNorm(num_groups=32, num_channels=dim)
        self.conv1 = Conv2d(dim, dim, 1, bias=False)
        self.gn1 = GroupNorm(num_groups=32, num_channels=dim)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv2 = ConvModule(dim, dim, kernel_size, stride=1, padding=(kernel_size - 1) // 2, conv_cfg=conv_cfg,
                                norm_cfg=norm_cfg)
        self.pool1, self.pool2 = pool1, pool2

    def forward(self, x):
        a, b = self.p1_conv1(x), self.p2_conv1(x)
        if type(self.pool1) is CornerPool and type(self.pool2) is CornerPool:
            pooled = corner_pool_sum(a, self.pool1.mode, b, self.pool2.mode)
        else:
            pooled = self.pool1(a) + self.pool2(b)
        return self.conv2(self.relu1(self.p_gn1(self.p_conv1(pooled)) + self.gn1(self.conv1(x))))


class TLPool(CornerPoolPack):

    def __init__(self, dim, conv_cfg=None, norm_cfg=None, first_kernel_size=3, kernel_size=3, corner_dim=128):
        super().__init__(dim, CornerPool('top'), CornerPool('left'), conv_cfg, norm_cfg, first_kernel_size,
                         kernel_size, corner_dim)


class BRPool(CornerPoolPack):

    def __init__(self, dim, conv_cfg=None, norm_cfg=None, first_kernel_size=3, kernel_size=3, corner_dim=128):
        super().__init__(dim, CornerPool('bottom'), CornerPool('right'), conv_cfg, norm_cfg, first_kernel_size,
                         kernel_size, corner_dim)
