"""Pooling and resampling around the convolutions: max pool (ResNet stem, FPN extra levels), average pool (Res2Net), the FPN's
nearest upsample + add.  Corner pooling, the fourth member of the family, lives in ops/corner_pool.py.

On the device these run as kernels of the library (lsn_max_pool2d_* / lsn_avg_pool2d_* / lsn_upsample_add_*: csrc/pool.hip,
index, tie and divisor rules in csrc/pool_rows.h): fp32 channels-last tensors -- or channel slices of one, read in place
through their pixel pitch -- with C % 4 == 0.  The forward values are the bits ATen returns (a maximum and a single add are
exact; the average divides the row-major window sum); every backward sums in a fixed order without atomics.  Anything else
-- host tensors, other dtypes and layouts, shapes the library refuses, LSNET_NATIVE_POOL=0 -- runs the framework's statements
as before.

For the average pool those statements are `avg_pool_nchw`, both passes on dense NCHW copies: ATen's avg_pool2d BACKWARD for
channels-last tensors is wrong on this stack (torch 2.10 + ROCm 7): kernel 3 / stride 2 / padding 1 returns a gradient off by
0.68 of its range, for a dense channels-last input and for a strided channel slice alike, while the NCHW kernel agrees with
the host bit for bit (tests/test_ops_gpu.py::test_avg_pool_backward).  Found by the round-4 Res2Net gradient fixture
(tools/dbg_res2net.py): the pooled scale of every layerN.0 Bottle2neck was off by 0.86 of its range on the device while the
three convolved scales agreed with the host to 8e-7.  The reference's Res2Net runs its pools in NCHW
(mmdet/models/backbones/res2net.py:80-99, 213-231)."""
import os

import torch
import torch.nn.functional as F

from .backend import get_backend

_CL = torch.channels_last
# LSNET_NATIVE_POOL=0: the framework's statements on the device too (A/B switch; the tests compare the two)
NATIVE_POOL = os.environ.get('LSNET_NATIVE_POOL', '1') != '0'


def _pair(v):
    return list(v) if isinstance(v, (tuple, list)) else [v, v]


def _square(v):
    """the single int the library takes for a stride / padding given as an int or an equal pair, else None"""
    a, b = _pair(v)
    return int(a) if a == b and isinstance(a, int) else None


def _pitched(t):
    """`t` can be handed to the pooling kernels as it lies in memory"""
    from .hip_backend import pool_pitch
    p = pool_pitch(t)
    return p is not None and p % 4 == 0 and t.data_ptr() % 16 == 0


def native_ok(*tensors):
    """The library's pooling kernels take these tensors: CUDA fp32, (a channel slice of) channels-last, C % 4 == 0."""
    if not NATIVE_POOL:
        return False
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.numel() > 0
                and t.shape[1] % 4 == 0 and t.numel() < (1 << 33) and _pitched(t)):
            return False
    return True


def _grad_arg(g):
    """an incoming gradient as the kernels read it (autograd may hand over any layout)"""
    return g if (g.dtype == torch.float32 and _pitched(g)) else g.float().clone(memory_format=_CL)


def _fallback(what, x, detail):
    if NATIVE_POOL:
        from .conv import _warn_aten_fallback
        _warn_aten_fallback(what, x, detail)


def _describe(*ts):
    return ', '.join(f'{tuple(t.shape)} {t.dtype} strides {t.stride()}' for t in ts)


# ---- max pool --------------------------------------------------------------------------------------------------------
class _MaxPoolFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, kernel, stride, pad):
        be = get_backend(x)
        need = ctx.needs_input_grad[0] and kernel != (1, 1)
        y, slot = be.max_pool2d_forward(x, kernel, stride, pad, want_slot=need)
        ctx.cfg = (tuple(x.shape), kernel, stride, pad)
        ctx.save_for_backward(*([slot] if need else []))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        shape, kernel, stride, pad = ctx.cfg
        slot = ctx.saved_tensors[0] if ctx.saved_tensors else None
        go = _grad_arg(go)
        return get_backend(go).max_pool2d_backward(go, slot, shape, kernel, stride, pad), None, None, None


def max_pool2d(x, kernel_size, stride=None, padding=0):
    """F.max_pool2d(x, kernel_size, stride, padding): the first maximum of a window wins, a NaN propagates."""
    kernel = tuple(_pair(kernel_size))
    s, p = _square(kernel_size if stride is None else stride), _square(padding)
    if native_ok(x) and s is not None and p is not None and s > 0 and all(isinstance(k, int) and 2 * p <= k for k in kernel) \
            and kernel[0] * kernel[1] <= 255 and x.shape[2] + 2 * p >= kernel[0] and x.shape[3] + 2 * p >= kernel[1]:
        return _MaxPoolFn.apply(x, kernel, s, p)
    _fallback('max_pool2d', x, f'window {kernel}, stride {stride}, padding {padding}, input {_describe(x)}')
    return F.max_pool2d(x, kernel_size, stride, padding)


def max_pool(x, pool):
    """`pool(x)` for an nn.MaxPool2d module."""
    if pool.dilation in (1, (1, 1)) and not pool.ceil_mode and not pool.return_indices:
        return max_pool2d(x, pool.kernel_size, pool.stride, pool.padding)
    return pool(x)


# ---- average pool ----------------------------------------------------------------------------------------------------
class _AvgPoolNCHW(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, k, s, p, ceil_mode, count_include_pad):
        xc = x.contiguous()
        ctx.cfg = (k, s, p, ceil_mode, count_include_pad)
        ctx.save_for_backward(xc)
        return F.avg_pool2d(xc, k, s, p, ceil_mode, count_include_pad)

    @staticmethod
    def backward(ctx, go):
        (xc,) = ctx.saved_tensors
        k, s, p, ceil_mode, count_include_pad = ctx.cfg
        gx = torch.ops.aten.avg_pool2d_backward(go.contiguous(), xc, _pair(k), _pair(s), _pair(p), ceil_mode,
                                                count_include_pad, None)
        return gx, None, None, None, None, None


def avg_pool_nchw(x, pool):
    """`pool(x)` for an nn.AvgPool2d module, forward and backward through the NCHW kernels."""
    s = pool.stride if pool.stride is not None else pool.kernel_size
    return _AvgPoolNCHW.apply(x, pool.kernel_size, s, pool.padding, bool(pool.ceil_mode), bool(pool.count_include_pad))


class _AvgPoolFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, kernel, stride, pad, ceil_mode, count_include_pad):
        ctx.cfg = (tuple(x.shape), kernel, stride, pad, ceil_mode, count_include_pad)
        return get_backend(x).avg_pool2d_forward(x, kernel, stride, pad, ceil_mode, count_include_pad)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        shape, kernel, stride, pad, ceil_mode, count_include_pad = ctx.cfg
        go = _grad_arg(go)
        gx = get_backend(go).avg_pool2d_backward(go, shape, kernel, stride, pad, ceil_mode, count_include_pad)
        return gx, None, None, None, None, None


def avg_pool2d(x, kernel_size, stride=None, padding=0, ceil_mode=False, count_include_pad=True):
    """F.avg_pool2d(x, ...) with ATen's output size and divisor rules; the result is channels-last on the native path."""
    kernel = tuple(_pair(kernel_size))
    s, p = _square(kernel_size if stride is None else stride), _square(padding)
    if native_ok(x) and s is not None and p is not None and s > 0 and all(isinstance(k, int) and 2 * p <= k for k in kernel) \
            and kernel[0] * kernel[1] <= 255 and x.shape[2] + 2 * p >= kernel[0] and x.shape[3] + 2 * p >= kernel[1]:
        return _AvgPoolFn.apply(x, kernel, s, p, bool(ceil_mode), bool(count_include_pad))
    _fallback('avg_pool2d', x, f'window {kernel}, stride {stride}, padding {padding}, input {_describe(x)}')
    st = kernel_size if stride is None else stride
    return _AvgPoolNCHW.apply(x, kernel_size, st, padding, bool(ceil_mode), bool(count_include_pad))


def avg_pool(x, pool):
    """`pool(x)` for an nn.AvgPool2d module (Res2Net's pooled scale, the avg_down shortcuts)."""
    if pool.divisor_override is not None:
        return avg_pool_nchw(x, pool)
    return avg_pool2d(x, pool.kernel_size, pool.stride, pool.padding, pool.ceil_mode, pool.count_include_pad)


# ---- FPN top-down step -------------------------------------------------------------------------------------------------
class _UpsampleAddFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, top, lat):
        ctx.top_shape = tuple(top.shape)
        return get_backend(lat).upsample_add_forward(top, lat)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        g = _grad_arg(go)
        gt = get_backend(g).upsample_add_backward(g, ctx.top_shape) if ctx.needs_input_grad[0] else None
        return gt, (go if ctx.needs_input_grad[1] else None)


def upsample_add(top, lat, upsample_cfg=None):
    """lat + F.interpolate(top, size of lat): the FPN's top-down step in one pass when the interpolation is the nearest
    doubling of every FPN pair (lat twice as large as top, or one less, per axis)."""
    cfg = dict(mode='nearest') if upsample_cfg is None else dict(upsample_cfg)
    if set(cfg) == {'mode'} and cfg['mode'] == 'nearest' and native_ok(top, lat) and top.shape[:2] == lat.shape[:2] \
            and all(big in (2 * small, 2 * small - 1) for small, big in zip(top.shape[2:], lat.shape[2:])):
        return _UpsampleAddFn.apply(top, lat)
    if 'scale_factor' in cfg:
        return lat + F.interpolate(top, **cfg)
    _fallback('upsample_add', lat, f'{cfg}, top {_describe(top)}, lateral {_describe(lat)}')
    return lat + F.interpolate(top, size=lat.shape[2:], **cfg)
