"""Dense convolution behind CONV_LAYERS['Conv2d'] (the reference: torch.nn.Conv2d through
mmcv/cnn/bricks/conv.py:11-43 `build_conv_layer`).

`Conv2d` subclasses nn.Conv2d (same parameters and state-dict keys).  Every dense (groups = 1) convolution of a CUDA
channels-last fp32 tensor -- forward, data gradient (any stride), weight and bias gradient -- runs the split-bf16
implicit-GEMM kernels of csrc/conv_kernels.h in the library's math modes 'bf16x6' (fp32-equivalent, the default) and
'bf16x3'.  The kernels read weights as prepared images (MFMA fragment order); `weight_image` (ops/weight_images.py) keeps
one per (weight tensor, pass) and rebuilds it when the tensor's version counter moves, i.e. once per optimizer step.  Grouped
convolutions with 4 .. 32 channels per group (ResNeXt 64x4d bottlenecks) run the exact-fp32 kernels of csrc/gconv.hip
in every math mode.  Contiguous (NCHW) inputs are re-laid channels-last and LSN_MATH_FP32 runs the same fp32-equivalent
kernels: no vendor convolution is reached from a CUDA fp32 tensor.  Other group shapes, dtypes and CPU tensors go to ATen's
convolution, which is a different operator, not a fallback of the HIP path."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._lib import ptr, stream
from . import grad_sink
# (the cache's public names stay importable from here: the runner, the reducer, ops/resblock.py's `K` and tests take them here)
from .weight_images import SIDE_STREAM_IMAGES, _fold_bn, invalidate_weight_images, parameters_updated, weight_image  # noqa: F401

_CL = torch.channels_last


_warned_fallbacks = set()


def _warn_aten_fallback(what, x, detail):
    """A device tensor that leaves the library's own kernels for ATen (MIOpen on the device): legal -- shapes the kernels do
    not serve, tensors of 2 GiB and more, other dtypes -- but never silent.  Once per (operator, reason)."""
    if not (torch.is_tensor(x) and x.is_cuda):
        return
    key = (what, detail)
    if key in _warned_fallbacks:
        return
    _warned_fallbacks.add(key)
    import warnings
    warnings.warn(f'lsnet_amd.{what}: no HIP kernel of this library serves this call on {x.device} ({detail}); '
                  'falling back to the ATen operator', RuntimeWarning, stacklevel=3)


def _pad_channels(t, c_to, pad=0):
    """Zero-pad dim 1 of a 4-D tensor to `c_to` channels (and dims 2, 3 by `pad` on either side), in channels-last memory."""
    B, C, H, W = t.shape
    out = t.new_zeros((B, c_to, H + 2 * pad, W + 2 * pad)).contiguous(memory_format=_CL)
    out[:, :C, pad:pad + H, pad:pad + W] = t
    return out


def _pad_in_channels(x, weight, pad=0):
    """Input channels rounded up to a multiple of 4 (the 3-channel image of the stem: one zero channel and a zero column of
    taps), the image zero-padded by `pad` pixels as well.  -> (padded x, padded weight)"""
    C4 = (x.shape[1] + 3) // 4 * 4
    return _pad_channels(x, C4, pad), _pad_channels(weight, C4)


def _pad_narrow_co(w, gos):
    """Data gradient under few input channels: the narrow tiles read grad_output in 4-channel pieces, so a filter count that
    is no multiple of 4 is rounded up (zero filters are free).  -> (weight, gradients, Co) as the launch takes them."""
    Co, C, kh, kw = w.shape
    if not (Co % 4 and C <= 64):
        return w, gos, Co
    Co8 = (Co + 3) // 4 * 4
    gos8 = [_pad_channels(g, Co8) for g in gos]
    w8 = w.new_zeros((Co8, C, kh, kw)).contiguous(memory_format=_CL)
    w8[:Co] = w
    return w8, gos8, Co8


def _out_hw(H, W, kh, kw, stride, pad, dil):
    return (H + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1, (W + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1


def _forward_prepared(x, img, bias, w_shape, stride, pad, dil, relu, residual=None):
    """act(conv(x, the weight behind the prepared image `img`) + bias + residual) in one launch, one map."""
    B, C, H, W = x.shape
    Co, _, kh, kw = w_shape
    out = torch.empty((B, Co) + _out_hw(H, W, kh, kw, stride, pad, dil), device=x.device, dtype=torch.float32, memory_format=_CL)
    lv = (_lib.ConvLevel * 1)()
    lv[0].x, lv[0].out, lv[0].B, lv[0].H, lv[0].W, lv[0].residual = ptr(x), ptr(out), B, H, W, ptr(residual)
    _lib.check(_lib.load().lsn_conv2d_forward_prepared(1, lv, ptr(img), ptr(bias), C, C, Co, kh, kw, stride, pad, dil,
                                                       1 if relu else 0, stream()))
    return out


def _param_grad_buffers(w, bias, want_w, want_b):
    """Where a weight / bias gradient kernel writes: the parameters' gradient sinks (ops/grad_sink.py; accumulate = 1)
    when BOTH wanted gradients have one, fresh tensors otherwise (a grad_w scratch even when only the bias is wanted).
    Returns (the claim, grad_w buffer, grad_b buffer or None)."""
    c = grad_sink.claim([(w, want_w), (bias, want_b)], optional=(1,))
    if c.accumulate:
        return (c, *c.sinks)
    return c, torch.empty_like(w), (torch.empty(w.shape[0], device=w.device, dtype=torch.float32) if want_b else None)


# ---- kernel-level primitives (one C call each; the autograd Functions below and ops/resblock.py compose them) ----------
# LSNET_GATE_MULTI=0: one gate launch per map, on dense copies of sliced gradients (A/B switch)
GATE_MULTI = os.environ.get('LSNET_GATE_MULTI', '1') != '0'


def _images_apart(g):
    """Is g (B, C, H, W) a stack of dense channels-last images (whatever lies between them)?  -> floats between two images, or 0"""
    B, C, H, W = g.shape
    if g.dtype != torch.float32 or not g.is_cuda or g.data_ptr() % 16 or (C * H * W) % 4:
        return 0
    sb, sc, sh, sw = g.stride()
    if (C == 1 or sc == 1) and (W == 1 or sw == C) and (H == 1 or sh == W * C) and (B == 1 or (sb >= C * H * W and sb % 4 == 0)):
        return sb if B > 1 else C * H * W
    return 0


def relu_gate_multi(gys, ys):
    """[grad_y where y > 0 else 0] for the maps of one multi-level convolution in ONE launch (lsn_relu_gate_multi).  A gradient
    whose images lie apart -- a level sliced out of the head's concatenated tensor -- is read where it lies: no copy first."""
    n = len(gys)
    strides = [_images_apart(g) for g in gys]
    if not (0 < n <= 8 and all(strides) and all(y.is_contiguous(memory_format=_CL) and y.numel() % 4 == 0 and y.shape == g.shape
                                                 for g, y in zip(gys, ys))):
        gys = [g.contiguous(memory_format=_CL) for g in gys]
        return [relu_gate(g, o) if o.numel() % 4 == 0 else g * (o > 0) for g, o in zip(gys, ys)]
    outs = [torch.empty_like(y) for y in ys]
    jobs = (_lib.GateJob * n)()
    for j, (g, y, o, sb) in enumerate(zip(gys, ys, outs, strides)):
        jobs[j].grad_y, jobs[j].y, jobs[j].grad = g.data_ptr(), y.data_ptr(), o.data_ptr()
        jobs[j].B, jobs[j].per_image, jobs[j].gy_batch_stride = y.shape[0], y.numel() // y.shape[0], sb
    _lib.check(_lib.load().lsn_relu_gate_multi(n, jobs, stream()))
    return outs


def relu_gate(gy, y):
    """grad_y where y > 0, else 0 -- the gradient through a ReLU whose output was stored (lsn_relu_gate)."""
    g = torch.empty_like(y, memory_format=_CL)
    _lib.check(_lib.load().lsn_relu_gate(ptr(gy), ptr(y), ptr(g), y.numel(), stream()))
    return g


def dgrad(g, w, in_shape, stride, pad, dil, bn=None, residual=None, gate=None, out=None):
    """Data gradient of conv(x, w [scaled by the folded eval-mode BatchNorm `bn`]) under the upstream gradient g
    (channels-last).  In the epilogue of the launch: `residual` (another path's gradient of the same tensor; may be
    `out` itself) is added and `gate` (the stored ReLU output whose gradient this is) zeroes the closed elements."""
    B, C, H, W = in_shape
    Co, _, kh, kw = w.shape
    if out is None:
        out = torch.empty(in_shape, device=g.device, dtype=torch.float32, memory_format=_CL)
    lv = (_lib.ConvLevel * 1)()
    lv[0].x, lv[0].out, lv[0].B, lv[0].H, lv[0].W = ptr(g), ptr(out), B, H, W
    lv[0].residual, lv[0].gate = ptr(residual), ptr(gate)
    _lib.check(_lib.load().lsn_conv2d_backward_data_prepared(1, lv, ptr(weight_image(w, 1, stride, pad, dil, bn=bn)), C, Co, kh,
                                                             kw, stride, pad, dil, stream()))
    return out


def wgrad_bn(x, g, w, bn, stride, pad, dil, need=(True, True, True)):
    """Parameter gradients of bn_eval(conv(x, w)) under g = the (gated) gradient w.r.t. the normalised output
    (lsn_conv2d_backward_weight_bn: exact for every gamma).  Accumulates into the three gradient sinks when all three
    parameters have one (returns (None, None, None) to autograd), else returns fresh (grad_w, grad_gamma, grad_beta)
    with None for the entries `need` does not ask for."""
    B, C, H, W = x.shape
    Co, _, kh, kw = w.shape
    gamma, beta = bn.weight, bn.bias
    c = grad_sink.claim(list(zip((w, gamma, beta), need)))
    gw, dg, db = c.sinks if c.accumulate else (torch.empty_like(w), torch.empty_like(gamma), torch.empty_like(beta))
    _lib.check(_lib.load().lsn_conv2d_backward_weight_bn(
        ptr(x), ptr(g), ptr(w), ptr(gamma), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps), ptr(gw),
        ptr(dg), ptr(db), B, H, W, C, Co, kh, kw, stride, pad, dil, c.accumulate, stream()))
    return c.results((gw, dg, db))


def wgrad_bn_deferrable(w, bn):
    """Can this layer's parameter gradients be produced LATER, by a launch shared with other layers (wgrad_bn_jobs)?  Only
    into gradient sinks: autograd wants a returned gradient now."""
    return bool(grad_sink.claim([(w, True), (bn.weight, True), (bn.bias, True)]).accumulate and w.is_cuda)


def wgrad_bn_jobs(jobs, stride, pad, dil):
    """jobs: [(x, g, w, bn)] of ONE geometry, every parameter with a sink (wgrad_bn_deferrable): one launch
    (lsn_conv2d_backward_weight_bn_jobs) adds every job's (grad_w, grad_gamma, grad_beta) to its sinks."""
    x0, _, w0, _ = jobs[0]
    B, C, H, W = x0.shape
    Co, _, kh, kw = w0.shape
    lib = _lib.load()
    claims = [grad_sink.claim([(w, True), (bn.weight, True), (bn.bias, True)]) for _, _, w, bn in jobs]
    assert all(c.accumulate for c in claims), 'wgrad_bn_jobs: a job whose parameters lost their sinks'
    for i in range(0, len(jobs), 8):
        part = jobs[i:i + 8]
        arr = (_lib.WgradBnJob * len(part))()
        for q, (x, g, w, bn), c in zip(arr, part, claims[i:i + 8]):
            assert x.shape == x0.shape and w.shape == w0.shape
            q.x, q.g, q.w = ptr(x), ptr(g), ptr(w)
            q.bn_gamma, q.bn_mean, q.bn_var, q.bn_eps = ptr(bn.weight), ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps)
            q.grad_w, q.grad_gamma, q.grad_beta = map(ptr, c.sinks)
        _lib.check(lib.lsn_conv2d_backward_weight_bn_jobs(len(part), arr, B, H, W, C, Co, kh, kw, stride, pad, dil, 1, stream()))
    for c in claims:
        c.results()


def conv_fwd_bn(x, w, bn, stride, pad, dil, relu, residual=None):
    """act(bn_eval(conv(x, w)) + residual) in one launch (the norm folded into the prepared image)."""
    img, shift = weight_image(w, 0, bn=bn)
    return _forward_prepared(x, img, shift, w.shape, stride, pad, dil, relu, residual)


class _ConvFn(torch.autograd.Function):
    """Forward, data gradient (any stride: residue classes of the transposed convolution), weight and bias gradient:
    all through liblsnet_hip.so.  Needs C % 4 == 0 (`conv2d` pads the 3-channel stem input)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, relu):
        w = w.contiguous(memory_format=_CL)
        out = _forward_prepared(x, weight_image(w, 0), bias, w.shape, stride, pad, dil, relu)
        ctx.save_for_backward(x, w, out if relu else None)
        ctx.cfg = (stride, pad, dil, relu, bias is not None)
        ctx.bias_ref = bias    # (not saved for its value: backward only asks where its gradient goes)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        x, w, out = ctx.saved_tensors
        stride, pad, dil, relu, has_bias = ctx.cfg
        lib = _lib.load()
        go = go.contiguous(memory_format=_CL)
        if relu:
            go = relu_gate(go, out) if out.numel() % 4 == 0 else go * (out > 0)
        B, C, H, W = x.shape
        Co, _, kh, kw = w.shape
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            w8, (go8,), _ = _pad_narrow_co(w, [go])
            gx = dgrad(go8, w8, x.shape, stride, pad, dil)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            # weight gradient and the bias gradient in one pass over grad_output
            want_b = has_bias and ctx.needs_input_grad[2]
            c, gw, gb = _param_grad_buffers(w, ctx.bias_ref, ctx.needs_input_grad[1], want_b)
            _lib.check(lib.lsn_conv2d_backward_weight(ptr(x), ptr(go), ptr(gw), ptr(gb), B, H, W, C, Co, kh, kw, stride, pad,
                                                      dil, c.accumulate, stream()))
            gw, gb = c.results((gw, gb))
        return gx, gw, gb, None, None, None, None


class _GroupConvFn(torch.autograd.Function):
    """Grouped convolution (ResNeXt): forward, data gradient, weight / bias gradient through csrc/gconv.hip."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, groups):
        lib = _lib.load()
        B, C, H, W = x.shape
        Co, _, kh, kw = w.shape
        w = w.contiguous(memory_format=_CL)
        out = torch.empty((B, Co) + _out_hw(H, W, kh, kw, stride, pad, dil), device=x.device, dtype=torch.float32, memory_format=_CL)
        _lib.check(lib.lsn_grouped_conv2d_forward(ptr(x), ptr(w), ptr(bias), ptr(out), B, H, W, C, Co, kh, kw, stride, pad, dil,
                                                  groups, 0, stream()))
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad, dil, groups, bias is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        x, w = ctx.saved_tensors
        stride, pad, dil, groups, has_bias = ctx.cfg
        lib = _lib.load()
        go = go.contiguous(memory_format=_CL)
        B, C, H, W = x.shape
        Co, _, kh, kw = w.shape
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x, memory_format=_CL)
            _lib.check(lib.lsn_grouped_conv2d_backward_data(ptr(go), ptr(w), ptr(gx), B, H, W, C, Co, kh, kw, stride, pad, dil,
                                                            groups, stream()))
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gw = torch.empty_like(w)
            gb = torch.empty(Co, device=x.device, dtype=torch.float32) if has_bias and ctx.needs_input_grad[2] else None
            _lib.check(lib.lsn_grouped_conv2d_backward_weight(ptr(x), ptr(go), ptr(gw), ptr(gb), B, H, W, C, Co, kh, kw, stride,
                                                              pad, dil, groups, 0, stream()))
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb, None, None, None, None


def hip_group_conv_ok(x, weight, stride, padding, dilation, groups, padding_mode='zeros'):
    """Shapes the grouped kernels take (include/lsnet_hip.h): in = out = 4, 8, 16 or 32 channels per group, <= 9 taps."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(memory_format=_CL)):
        return False
    if groups <= 1 or padding_mode != 'zeros' or isinstance(padding, str):
        return False
    if stride[0] != stride[1] or padding[0] != padding[1] or dilation[0] != dilation[1]:
        return False
    Co, cg, kh, kw = weight.shape
    if x.shape[1] != cg * groups or Co != cg * groups or cg not in (4, 8, 16, 32) or kh * kw > 9:
        return False
    return x.numel() < 2 ** 31 and Co * x.shape[0] * x.shape[2] * x.shape[3] < 2 ** 31


def conv_multi_fwd(xs, w, bias, pad, dil, relu, residuals=None):
    """[conv2d(x, w, bias, 1, pad, dil) for x in xs] in ONE launch (channels-last device tensors; no autograd).
    residuals: per-map tensors of the outputs' shape, added in the epilogue (before the ReLU, lsn_conv_level.residual)."""
    Co, C, kh, kw = w.shape
    n = len(xs)
    levels = (_lib.ConvLevel * n)()
    outs = []
    for i, x in enumerate(xs):
        B, _, H, W = x.shape
        out = torch.empty((B, Co) + _out_hw(H, W, kh, kw, 1, pad, dil), device=x.device, dtype=torch.float32, memory_format=_CL)
        outs.append(out)
        L = levels[i]
        L.x, L.out, L.B, L.H, L.W = ptr(x), ptr(out), B, H, W
        if residuals is not None:
            assert residuals[i].shape == out.shape and residuals[i].is_contiguous(memory_format=_CL)
            L.residual = ptr(residuals[i])
    _lib.check(_lib.load().lsn_conv2d_forward_prepared(n, levels, ptr(weight_image(w, 0)), ptr(bias), C, C, Co, kh, kw, 1, pad, dil,
                                                       1 if relu else 0, stream()))
    return outs


def conv_multi_dgrad(gos, w, xs, pad, dil, accumulate_into=None):
    """Data gradients of conv_multi_fwd for every map in ONE launch.  accumulate_into: per-map tensors of the inputs' shape
    that already hold another path's gradient of the same input -- the results are ADDED to them in the epilogue of the
    launch (lsn_conv_level.residual aliasing out) and they are returned."""
    Co, C, kh, kw = w.shape
    n = len(xs)
    w8, gos8, Co8 = _pad_narrow_co(w, gos)
    levels = (_lib.ConvLevel * n)()
    gxs = []
    for i, x in enumerate(xs):
        gx = accumulate_into[i] if accumulate_into is not None else torch.empty_like(x, memory_format=_CL)
        gxs.append(gx)
        L = levels[i]
        L.x, L.out, L.B, L.H, L.W = ptr(gos8[i]), ptr(gx), x.shape[0], x.shape[2], x.shape[3]
        if accumulate_into is not None:
            L.residual = ptr(gx)
    _lib.check(_lib.load().lsn_conv2d_backward_data_prepared(n, levels, ptr(weight_image(w8, 1, 1, pad, dil)), C, Co8, kh, kw, 1,
                                                             pad, dil, stream()))
    return gxs


def conv_multi_wgrad(xs, gos, w, bias, pad, dil, want_w=True, want_b=True):
    """Weight / bias gradient summed over the maps in ONE launch; into the parameters' gradient sinks when they have them
    (then (None, None) goes back to autograd)."""
    Co, C, kh, kw = w.shape
    n = len(xs)
    levels = (_lib.ConvLevel * n)()
    for i, x in enumerate(xs):
        L = levels[i]
        L.x, L.grad_out, L.B, L.H, L.W = ptr(x), ptr(gos[i]), x.shape[0], x.shape[2], x.shape[3]
    want_b = want_b and bias is not None
    c, gw, gb = _param_grad_buffers(w, bias, want_w, want_b)
    _lib.check(_lib.load().lsn_conv2d_backward_weight_multi(n, levels, ptr(gw), ptr(gb), C, Co, kh, kw, 1, pad, dil, c.accumulate,
                                                            stream()))
    return c.results((gw, gb))


class _ConvMultiFn(torch.autograd.Function):
    """Several input maps of different sizes under ONE weight (the FPN levels of LSHead's shared convolutions):
    forward, data gradients and the weight / bias gradient (summed over the maps) in one launch each.  Stride 1."""

    @staticmethod
    def forward(ctx, w, bias, cfg, *xs):
        pad, dil, relu = cfg[:3]
        nres = cfg[3] if len(cfg) > 3 else 0     # the last nres tensors are residuals of the first maps' outputs (round 5)
        res = list(xs[len(xs) - nres:]) if nres else None
        xs = xs[:len(xs) - nres] if nres else xs
        w = w.contiguous(memory_format=_CL)
        outs = conv_multi_fwd(xs, w, bias, pad, dil, relu, res)
        ctx.save_for_backward(w, *xs, *(outs if relu else []))
        ctx.cfg, ctx.n, ctx.has_bias, ctx.nres = (pad, dil, relu), len(xs), bias is not None, nres
        ctx.bias_ref = bias
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gos):
        pad, dil, relu = ctx.cfg
        n = ctx.n
        saved = ctx.saved_tensors
        w, xs = saved[0], saved[1:1 + n]
        outs = saved[1 + n:] if relu else None
        if relu and GATE_MULTI:
            gos = relu_gate_multi(list(gos), outs)      # one launch for all maps, reading sliced gradients where they lie
        elif relu:
            gos = [g.contiguous(memory_format=_CL) for g in gos]
            gos = [relu_gate(g, o) if o.numel() % 4 == 0 else g * (o > 0) for g, o in zip(gos, outs)]
        else:
            gos = [g.contiguous(memory_format=_CL) for g in gos]
        need_x = [ctx.needs_input_grad[3 + i] for i in range(n)]
        gxs = [None] * n
        if any(need_x):
            gxs = [g if need else None for g, need in zip(conv_multi_dgrad(gos, w, xs, pad, dil), need_x)]
        gw = gb = None
        if ctx.needs_input_grad[0] or (ctx.has_bias and ctx.needs_input_grad[1]):
            gw, gb = conv_multi_wgrad(xs, gos, w, ctx.bias_ref, pad, dil, ctx.needs_input_grad[0],
                                      ctx.has_bias and ctx.needs_input_grad[1])
        # the residual sits in front of the ReLU: its gradient is the (gated) output gradient itself
        gres = [gos[i] if ctx.needs_input_grad[3 + n + i] else None for i in range(ctx.nres)]
        return (gw, gb, None, *gxs, *gres)


def conv2d_multi(xs, weight, bias=None, padding=0, dilation=1, relu=False, residuals=None):
    """[conv2d(x, weight, bias, 1, padding, dilation) (+ residual) for x in xs] in one launch per pass (stride 1, up to 8 maps).
    residuals: one tensor of the output's shape per map, added in the launch's epilogue (before the ReLU) -- the sum of two
    branches without an element-wise launch of its own (LSHead's `relu(1x1(gathered)) + 3x3(tower)`, lsnet_head.py:640-755)."""
    nres = 0 if residuals is None else len(residuals)
    assert nres in (0, len(xs))
    return list(_ConvMultiFn.apply(weight, bias, (int(padding), int(dilation), bool(relu), nres), *xs, *(residuals or [])))


def hip_conv_ok(x, weight, stride, padding, dilation, groups, padding_mode='zeros'):
    """The own kernels take every dense (groups = 1) fp32 convolution on the device, in every math mode and memory
    format: a contiguous (NCHW) tensor is re-laid channels-last on the way in (`_as_cl`, a layout copy -- the result stays
    channels-last, as ATen's own convolution propagates the format), and LSN_MATH_FP32 runs the fp32-EQUIVALENT 6-term
    kernels here (exactness of that mode concerns the deformable family; there is no fp32-MFMA dense kernel, and no vendor
    convolution is called either).  What is left for F.conv2d: other dtypes / devices, 'same' / non-zero padding modes,
    unequal strides, tensors beyond 32-bit byte offsets."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
        return False
    if groups != 1 or padding_mode != 'zeros' or isinstance(padding, str):
        return False
    if stride[0] != stride[1] or padding[0] != padding[1] or dilation[0] != dilation[1]:
        return False
    if x.numel() * 4 >= 2 ** 31 or weight.numel() * 8 >= 2 ** 31 or weight.shape[2] * weight.shape[3] > 64:
        return False
    # the output (and with it grad_output of the backward passes) must fit 32-bit byte offsets too: csrc/conv.hip conv_check
    kh, kw = weight.shape[2], weight.shape[3]
    ho, wo = _out_hw(x.shape[2], x.shape[3], kh, kw, stride[0], padding[0], dilation[0])   # (equal along both axes: above)
    if ho <= 0 or wo <= 0 or x.shape[0] * ho * wo * weight.shape[0] * 4 >= 2 ** 31:
        return False
    return True


def _as_cl(x):
    return x if x.is_contiguous(memory_format=_CL) else x.contiguous(memory_format=_CL)


def _stem_forward(x, weight, bias, stride, pad, relu):
    """Forward of a shallow wide-kernel convolution (the 7x7 stem on the 3-channel image) in the row-merged form of
    lsn_conv2d_forward_pitched: the image is zero-padded (space: `pad`, channels: to 4) once, then a tap row of kw
    pixels x 4 channels is ONE contiguous 4 kw-float "channel" run -- kh chunks of the implicit GEMM instead of kh * kw
    chunks that are 1/8 full.  No gradient (the stem is frozen in every LSNet config)."""
    B, _, H, W = x.shape
    Co, _, kh, kw = weight.shape
    xp, w4 = _pad_in_channels(x, weight, pad)     # w4's memory: (Co, kh, kw, C4) = (Co, kh, 1, kw C4)
    C4 = w4.shape[1]
    out = torch.empty((B, Co) + _out_hw(H, W, kh, kw, stride, pad, 1), device=x.device, dtype=torch.float32, memory_format=_CL)
    _lib.check(_lib.load().lsn_conv2d_forward_pitched(ptr(xp), ptr(w4), ptr(bias), ptr(out), None, B, H + 2 * pad, W + 2 * pad,
                                                      kw * C4, C4, Co, kh, 1, stride, 0, 1, 1 if relu else 0, stream()))
    return out


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, relu=False):
    C = x.shape[1]
    no_grad = not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or
                                                (bias is not None and bias.requires_grad)))
    if C < 8 and weight.shape[3] > 1 and int(dilation) == 1 and no_grad:
        return _stem_forward(x, weight, bias, int(stride), int(padding), bool(relu))
    if C % 4:    # the 3-channel image of the stem: one zero channel (and a zero column of taps)
        x, weight = _pad_in_channels(x, weight)
    return _ConvFn.apply(x, weight, bias, int(stride), int(padding), int(dilation), bool(relu))


def conv_bn_act_frozen(conv, bn, x, relu=True, residual=None):
    """relu(bn(conv(x)) + residual) in ONE launch for a FROZEN conv + eval-mode BatchNorm pair whose input needs no
    gradient (stem and stage 1 of every LSNet backbone, `frozen_stages=1`: resnet.py:569-585, 636-645): the norm is folded
    into the weight / bias, residual add and ReLU ride in the convolution's epilogue (include/lsnet_hip.h
    lsn_conv_level.residual) -- no normalisation pass over the largest activations of the network.  Returns None when the
    pair does not qualify (the caller then runs conv and bn_act separately)."""
    if not isinstance(conv, Conv2d) or conv.bias is not None or conv.groups != 1 or bn.training or not bn.affine \
            or not bn.track_running_stats:
        return None
    if conv.weight.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad \
            or (torch.is_grad_enabled() and x.requires_grad):
        return None
    if not hip_conv_ok(x, conv.weight, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode):
        return None
    x = _as_cl(x)
    w, shift = _fold_bn(conv, bn)
    stride, pad, dil = conv.stride[0], conv.padding[0], conv.dilation[0]
    B, C, H, W = x.shape
    Co, _, kh, kw = w.shape
    if C < 8:    # the image stem: row-merged form, no residual there
        if residual is not None or kw == 1 or dil != 1:
            return None
        return _stem_forward(x, w, shift, stride, pad, relu)
    if C % 4:
        return None
    if residual is not None:
        if not (tuple(residual.shape) == (B, Co) + _out_hw(H, W, kh, kw, stride, pad, dil) and residual.dtype == torch.float32
                and Co % 4 == 0):
            return None
        residual = _as_cl(residual)
    return _forward_prepared(x, weight_image(w, 0), shift, w.shape, stride, pad, dil, relu, residual)


class _ConvBnActFn(torch.autograd.Function):
    """y = act(bn(conv(x)) + residual) with the eval-mode BatchNorm FOLDED into the convolution (one launch, the raw
    convolution output is never stored) and every gradient -- input, residual, weight, gamma, beta -- from the library.
    Backward: g = ReLU gate of grad_y (one streaming pass; g is also the residual's gradient); the data gradient runs
    on the backward image of the SCALED weight; lsn_conv2d_backward_weight_bn forms grad_w, grad_gamma and grad_beta from
    ONE weight-gradient launch with conv = w . x pulled out of the pixel sum -- exact for every gamma (a zero-initialised
    norm3, `zero_init_residual`, learns; nothing is divided by gamma)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, residual, bn, stride, pad, dil, relu):
        out = conv_fwd_bn(x, w, bn, stride, pad, dil, relu, residual)
        ctx.save_for_backward(x, w, out if relu else None)
        ctx.cfg = (stride, pad, dil, relu, residual is not None)
        ctx.bn = bn
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        stride, pad, dil, relu, has_res = ctx.cfg
        bn = ctx.bn
        gy = gy.contiguous(memory_format=_CL)
        need_x, need_w, need_g, need_b = ctx.needs_input_grad[:4]
        need_res = has_res and ctx.needs_input_grad[4]
        g = relu_gate(gy, y) if relu else gy
        gx = gw = dg = db = None
        if need_x:
            gx = dgrad(g, w, x.shape, stride, pad, dil, bn=bn)
        if need_w or need_g or need_b:
            gw, dg, db = wgrad_bn(x, g, w, bn, stride, pad, dil, (need_w, need_g, need_b))
        return gx, gw, dg, db, (g if need_res else None), None, None, None, None, None


def conv_bn_act(conv, bn, x, relu=True, residual=None):
    """relu(bn(conv(x)) + residual) in ONE forward launch for a TRAINABLE convolution + eval-mode BatchNorm pair (stages
    2 - 4 of the LSNet backbones: `norm_eval=True` keeps the statistics fixed while gamma / beta train,
    resnet.py:636-645): the norm's scale is folded into the weight image that is rebuilt after every optimizer step
    anyway, its shift rides in the bias slot, residual add and ReLU in the epilogue.  Saves the normalisation pass over
    every backbone activation (a read and a write) and the storage of the raw convolution output.  Returns None when the
    pair does not qualify (the caller then runs conv and bn_act separately)."""
    if not isinstance(conv, Conv2d) or conv.bias is not None or conv.groups != 1 or bn.training or not bn.affine \
            or not bn.track_running_stats or not isinstance(bn, nn.BatchNorm2d):
        return None
    if not hip_conv_ok(x, conv.weight, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode):
        return None
    Co, C, kh, kw = conv.weight.shape
    if C % 4 or Co % 4 or not (256 % (Co // 4) == 0 if Co <= 1024 else Co % 1024 == 0):
        return None
    if not conv.weight.is_contiguous(memory_format=_CL):
        return None
    x = _as_cl(x)
    stride, pad, dil = conv.stride[0], conv.padding[0], conv.dilation[0]
    B, _, H, W = x.shape
    if residual is not None:
        if not (tuple(residual.shape) == (B, Co) + _out_hw(H, W, kh, kw, stride, pad, dil) and residual.dtype == torch.float32):
            return None
        residual = _as_cl(residual)
    return _ConvBnActFn.apply(x, conv.weight, bn.weight, bn.bias, residual, bn, stride, pad, dil, bool(relu))


class Conv2d(nn.Conv2d):

    def forward(self, x, weight=None):
        """`weight`: use this tensor instead of the module's parameter (a zero-padded view of it, for inputs whose
        channel count was rounded up to the kernels' granularity)."""
        if weight is not None:
            return self._run(x, weight)
        return self._run(x, self.weight)

    def forward_multi(self, xs, relu=False, residuals=None):
        """The same convolution over several maps (FPN levels) in ONE launch per pass.  residuals: per-map tensors added to the
        outputs (before the ReLU) -- in the launch's epilogue on the device."""
        xs = list(xs)
        if (1 < len(xs) <= 8 and self.stride[0] == 1 and xs[0].shape[1] % 4 == 0
                and all(hip_conv_ok(x, self.weight, self.stride, self.padding, self.dilation, self.groups,
                                    self.padding_mode) for x in xs)
                and (residuals is None or (self.weight.shape[0] % 4 == 0 and all(r.is_cuda and r.dtype == torch.float32 for r in residuals)))):
            res = None if residuals is None else [_as_cl(r) for r in residuals]
            return conv2d_multi([_as_cl(x) for x in xs], self.weight, self.bias, self.padding[0], self.dilation[0], relu, res)
        outs = [self._run(x, self.weight) for x in xs]
        if residuals is not None:
            outs = [o + r for o, r in zip(outs, residuals)]
        return [F.relu(o) for o in outs] if relu else outs

    def _run(self, x, w):
        if hip_conv_ok(x, w, self.stride, self.padding, self.dilation, self.groups, self.padding_mode):
            return conv2d(_as_cl(x), w, self.bias, self.stride[0], self.padding[0], self.dilation[0], False)
        if hip_group_conv_ok(x, w, self.stride, self.padding, self.dilation, self.groups, self.padding_mode):
            return _GroupConvFn.apply(x, w, self.bias, self.stride[0], self.padding[0], self.dilation[0], self.groups)
        _warn_aten_fallback('Conv2d', x, f'weight {tuple(w.shape)}, stride {self.stride}, groups {self.groups}, '
                                           f'padding_mode {self.padding_mode}, input {tuple(x.shape)} {x.dtype}')
        return self._conv_forward(x, w, self.bias)     # (nn.Conv2d's own: F.conv2d behind the module's padding_mode)
