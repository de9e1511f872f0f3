"""One backbone stage per block variant, with a float64 reference that is a plain restatement of the blocks in torch.

Shared by tests/test_backbone_stages_host.py (the package's host path against the restatement) and
tests/test_backbone_stages_gpu.py (the device against the same numbers).  A case is a ResLayer / Res2Layer of two or three blocks
on a 2 x C x 15 x 13 input: the odd map gives the ceil_mode / count_include_pad=False average pools a partial window and a stride
of 2 an 8 x 7 output.  The stage is in train mode with every BatchNorm in eval(), as ResNet.train leaves it.

`stage_fp64` states every block against its formula -- F.conv2d, F.batch_norm(training=False) / F.group_norm, F.avg_pool2d with
each module's own flags, torch.split / cat and, for a deformable conv, F.conv2d of conv_offset followed by
tests/torch_dcn_ref.py::torch_dcn -- and never calls `_body`.  It runs in the dtype of the layer it is given.

The comparisons hold EVERY element of every gradient to a hard bound.  That is legitimate only because `build` moves the
parameters until two conditions hold in the float64 run, and the host test asserts them again:
  kink clearance     every ReLU input lies at least DELTA x (max-abs of its tensor) from zero: DELTA is the forward bound, so an
                     evaluation whose forward is within bound takes the same gates;
  lattice clearance  no sampling coordinate of a deformable conv lies within LATTICE of an integer (the borders -1, H and W
                     included), where the bilinear weights have their kinks and the inside test switches."""
import copy
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.torch_dcn_ref import torch_dcn

B, H, W = 2, 15, 13
DELTA = 1e-5        # kink clearance, as a share of the ReLU input's max-abs (= the forward bound)
LATTICE = 1e-5      # lattice clearance, in pixels
DCN2 = dict(type='DCNv2', deformable_groups=1, fallback_on_stride=False)
GN8 = dict(type='GN', num_groups=8, requires_grad=True)

# name: (layer class, block class, inplanes, planes, blocks, keyword arguments)
CASES = {
    # DCNv2 pack (27-channel offset/mask conv, modulated DCN), folded conv + BN around it, projection shortcut
    'r_v2_s2': ('ResLayer', 'Bottleneck', 64, 32, 3, dict(stride=2, dcn=DCN2)),
    # the stride in the 1x1 conv1, four deformable groups
    'r_v2_dg4_caffe': ('ResLayer', 'Bottleneck', 128, 64, 2, dict(stride=2, style='caffe', dcn=dict(DCN2, deformable_groups=4))),
    # DCNv1 (no mask), dilation 2, identity shortcut in block 0
    'r_v1_dil2': ('ResLayer', 'Bottleneck', 128, 32, 2,
                  dict(stride=1, dilation=2, dcn=dict(type='DCN', deformable_groups=1, fallback_on_stride=False))),
    # gconv.hip at 4 channels per group, strided
    'x_c4_s2': ('ResLayer', 'Bottleneck', 64, 64, 3, dict(stride=2, groups=16, base_width=4)),
    # gconv.hip at 32 channels per group, identity shortcut
    'x_c32_s1': ('ResLayer', 'Bottleneck', 256, 64, 2, dict(groups=2, base_width=32)),
    # grouped DCN kernels: width 64, 8 per group, strided
    'x_dcn_c8_s2': ('ResLayer', 'Bottleneck', 64, 32, 3, dict(stride=2, groups=8, base_width=16, dcn=DCN2)),
    # grouped DCN at width 128, 16 per group
    'x_dcn_c16_s1': ('ResLayer', 'Bottleneck', 256, 64, 2, dict(groups=8, base_width=16, dcn=DCN2)),
    # width 52: 'stage' block with the 3x3 pool of the last scale and the average-pool shortcut, then 'normal' blocks
    'r2_s2': ('Res2Layer', 'Bottle2neck', 128, 128, 3, dict(stride=2, scales=4, base_width=26)),
    # the headline backbone's DCN stage
    'r2_dcn_s2': ('Res2Layer', 'Bottle2neck', 128, 128, 3, dict(stride=2, scales=4, base_width=26, dcn=DCN2)),
    # 'stage' block without a pool; shortcut with a 1x1 stride-1 AvgPool2d in front
    'r2_dcn_s1': ('Res2Layer', 'Bottle2neck', 128, 128, 2, dict(stride=1, scales=4, base_width=26, dcn=DCN2)),
    # the ResNet-18 / 34 block
    'basic_s2': ('ResLayer', 'BasicBlock', 64, 128, 2, dict(stride=2)),
    # conv followed by the GroupNorm kernels instead of a folded BatchNorm
    'gn_s2': ('ResLayer', 'Bottleneck', 64, 32, 2, dict(stride=2, norm_cfg=GN8)),
}
DCN_CASES = [n for n, c in CASES.items() if 'dcn' in c[5]]
NORMS = (nn.modules.batchnorm._BatchNorm, nn.GroupNorm)


def make(name):
    """The stage as the package builds it (default initialisation), in train mode with its BatchNorms in eval()."""
    from lsnet_amd.models.backbones import res2net, resnet
    kind, block, inplanes, planes, n, kw = CASES[name]
    space = dict(ResLayer=resnet.ResLayer, Res2Layer=res2net.Res2Layer, Bottleneck=resnet.Bottleneck,
                 BasicBlock=resnet.BasicBlock, Bottle2neck=res2net.Bottle2neck)
    return as_trained(space[kind](space[block], inplanes, planes, n, **copy.deepcopy(kw)))


def as_trained(layer):
    layer.train()
    for m in layer.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.eval()
    for p in layer.parameters():
        p.requires_grad_(True)
    return layer


# ---- the float64 statement of the blocks ---------------------------------------------------------------------------------------
class Trace:
    """What the two conditions are about, in forward order: ('relu', name, input, name of the norm in front of it) and
    ('coord', name, sampling coordinates (B, dg 2 K, Ho, Wo) in offset-channel order, name of the conv_offset module)."""

    def __init__(self):
        self.events = []


def _first(v):
    return int(v[0] if isinstance(v, (tuple, list)) else v)


def sampling_coords(off, stride, pad, dil, kh, kw):
    """Absolute sampling positions of a deformable conv in the channel order of its offsets: channel d 2K + 2k is the row
    ho stride - pad + i dil + offset of tap k = (i, j), the next one the column."""
    Ho, Wo = off.shape[2:]
    K = kh * kw
    base = torch.zeros(2 * K, Ho, Wo, dtype=off.dtype)
    for k in range(K):
        i, j = divmod(k, kw)
        base[2 * k] = (torch.arange(Ho, dtype=off.dtype) * stride - pad + i * dil).view(Ho, 1)
        base[2 * k + 1] = (torch.arange(Wo, dtype=off.dtype) * stride - pad + j * dil).view(1, Wo)
    return off + base.repeat(off.shape[1] // (2 * K), 1, 1)


def stage_fp64(layer, x, trace=None, wrong=None):
    """The stage's output for input x, block by block against the formulas, in the dtype of `layer`.
    wrong: one of WRONG_STATEMENTS -- a deliberately wrong restatement (tests/test_backbone_stages_host.py uses them to show
    that the bound notices)."""
    from lsnet_amd.models.backbones.res2net import Bottle2neck
    from lsnet_amd.models.backbones.resnet import BasicBlock, Bottleneck
    from lsnet_amd.ops.dcn import ModulatedDeformConvPack
    names = {id(m): n for n, m in layer.named_modules()}

    def norm(m, t):
        if isinstance(m, nn.GroupNorm):
            return F.group_norm(t, m.num_groups, m.weight, m.bias, m.eps)
        return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)

    def relu(t, m, what):
        if trace is not None:
            trace.events.append(('relu', f'{names[id(m)]} -> {what}', t.detach(), names[id(m)]))
        return torch.relu(t)

    def conv(m, t):
        if not hasattr(m, 'conv_offset'):
            return F.conv2d(t, m.weight, m.bias, m.stride, m.padding, m.dilation, m.groups)
        co = m.conv_offset
        om = F.conv2d(t, co.weight, co.bias, co.stride, co.padding, co.dilation)
        kh, kw = m.kernel_size
        dg = m.deformable_groups
        stride, pad, dil = _first(m.stride), _first(m.padding), _first(m.dilation)
        n_off = 2 * dg * kh * kw
        off, mask = om, None
        if isinstance(m, ModulatedDeformConvPack):     # offsets | mask logits
            off, mask = om[:, :n_off], om[:, n_off:]
            if wrong != 'mask_without_sigmoid':
                mask = torch.sigmoid(mask)
        if trace is not None:
            trace.events.append(('coord', names[id(m)], sampling_coords(off.detach(), stride, pad, dil, kh, kw), names[id(co)]))
        if wrong == 'offsets_as_xy':
            off = off.reshape(off.shape[0], -1, 2, *off.shape[2:]).flip(2).reshape(off.shape)
        return torch_dcn(t, off, mask, m.weight, getattr(m, 'bias', None), stride, pad, dil, m.groups, dg)

    def shortcut(ds, t):
        if ds is None:
            return t
        for m in ds:
            if isinstance(m, nn.AvgPool2d):
                if wrong == 'shortcut_pool_full_divisor':
                    k = _first(m.kernel_size)
                    t = F.avg_pool2d(t, m.kernel_size, m.stride, m.padding, m.ceil_mode, True, divisor_override=k * k)
                else:
                    t = F.avg_pool2d(t, m.kernel_size, m.stride, m.padding, m.ceil_mode, m.count_include_pad)
            elif isinstance(m, NORMS):
                t = norm(m, t)
            else:
                t = conv(m, t)
        return t

    def basic(b, t):
        out = relu(norm(b.norm1, conv(b.conv1, t)), b.norm1, 'relu')
        return relu(norm(b.norm2, conv(b.conv2, out)) + shortcut(b.downsample, t), b.norm2, 'relu')

    def bottleneck(b, t):
        out = relu(norm(b.norm1, conv(b.conv1, t)), b.norm1, 'relu')
        out = relu(norm(b.norm2, conv(b.conv2, out)), b.norm2, 'relu')
        return relu(norm(b.norm3, conv(b.conv3, out)) + shortcut(b.downsample, t), b.norm3, 'relu')

    def bottle2neck(b, t):
        out = relu(norm(b.norm1, conv(b.conv1, t)), b.norm1, 'relu')
        spx = torch.split(out, b.width, 1)
        parts, sp = [], None
        for i in range(b.scales - 1):
            if i == 0 or b.stage_type == 'stage' or wrong == 'no_running_sum':
                sp = spx[i]
            else:
                sp = sp + spx[i]
            sp = relu(norm(b.bns[i], conv(b.convs[i], sp)), b.bns[i], 'relu')
            parts.append(sp)
        last = spx[b.scales - 1]
        if b.stage_type == 'stage' and b.conv2_stride != 1:
            p = b.pool
            last = F.avg_pool2d(last, p.kernel_size, p.stride, p.padding, p.ceil_mode, p.count_include_pad)
        out = torch.cat(parts + [last], 1)
        return relu(norm(b.norm3, conv(b.conv3, out)) + shortcut(b.downsample, t), b.norm3, 'relu')

    for b in layer:
        if isinstance(b, Bottle2neck):
            x = bottle2neck(b, x)
        elif isinstance(b, Bottleneck):
            x = bottleneck(b, x)
        else:
            assert isinstance(b, BasicBlock), type(b)
            x = basic(b, x)
    return x


# offsets read as (x, y); the Res2Net running sum left out; the shortcut pool's partial windows divided by the whole window
# (what count_include_pad=True is taken to mean: ATen itself clips the window to the padded map, so with padding 0 the flag alone
# changes nothing, and dropping ceil_mode changes the output's size); the v2 mask without its sigmoid.  -> a case that uses it
WRONG_STATEMENTS = {'offsets_as_xy': 'r_v2_s2', 'no_running_sum': 'r2_s2', 'shortcut_pool_full_divisor': 'r2_s2',
                    'mask_without_sigmoid': 'r_v2_s2'}


# ---- parameters -----------------------------------------------------------------------------------------------------------------
def violations(trace):
    """[(kind, event name, module to move, offending channels, step)] for the events of a float64 run that break a condition."""
    bad = []
    for kind, name, t, mod in trace.events:
        if kind == 'relu':
            top = float(t.abs().max())
            hit = t.abs() < DELTA * top
            step = 4 * DELTA * top
        else:
            hit = (t - t.round()).abs() < LATTICE
            step = 4 * LATTICE
        if bool(hit.any()):
            bad.append((kind, name, mod, hit.any(0).flatten(1).any(1).nonzero().flatten().tolist(), step))
    return bad


def build(name):
    """-> (the stage with its parameters filled from one seeded generator and moved until both conditions hold, the input,
    how many passes and nudged channels that took)"""
    layer = make(name)
    g = torch.Generator().manual_seed(20240 + list(CASES).index(name))
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    with torch.no_grad():
        for n, m in layer.named_modules():
            if n.endswith('conv_offset'):
                m.weight.copy_(randn(m.weight.shape) * 0.05)
                m.bias.copy_(randn(m.bias.shape) * 0.5)
            elif isinstance(m, NORMS):
                m.weight.copy_(rand(m.weight.shape) + 0.5)
                m.bias.copy_(randn(m.bias.shape) * 0.3)
                if hasattr(m, 'running_mean'):
                    m.running_mean.copy_(randn(m.running_mean.shape) * 0.5)
                    m.running_var.copy_(rand(m.running_var.shape) * 1.5 + 0.5)
            elif isinstance(getattr(m, 'weight', None), nn.Parameter):      # dense, grouped and deformable main weights
                m.weight.copy_(randn(m.weight.shape) * math.sqrt(2.0 / m.weight[0].numel()))
        last = layer[-1]
        last_norm = last.norm3 if hasattr(last, 'norm3_name') else last.norm2
        last_norm.weight[:4] = 0.0
        last_norm.weight[4:8] = 1e-6
    x = randn(B, CASES[name][2], H, W)
    passes = nudged = 0
    while True:
        passes += 1
        assert passes < 200, f'{name}: the conditions were not reached'
        trace = Trace()
        with torch.no_grad():
            stage_fp64(copy.deepcopy(layer).double(), x.double(), trace)
        bad = violations(trace)
        if not bad:
            return layer, x, passes, nudged
        kind, _, mod, channels, step = bad[0]
        with torch.no_grad():
            layer.get_submodule(mod).bias[channels] += step
        nudged += len(channels)


def evaluate(layer, x, go, wrong=None):
    """{'out': stage_fp64(layer, x), 'x': the input gradient under go, parameter name: its gradient}, detached."""
    layer = copy.deepcopy(layer)
    x = x.clone().requires_grad_()
    y = stage_fp64(layer, x, wrong=wrong)
    named = list(layer.named_parameters())
    grads = torch.autograd.grad(y, [x] + [p for _, p in named], go, allow_unused=True)
    res = {'out': y.detach(), 'x': grads[0]}
    res.update({k: (torch.zeros_like(p) if gr is None else gr) for (k, p), gr in zip(named, grads[1:])})
    return res


def deviation(a, ref):
    """max |a - ref| as a share of ref's range"""
    return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def bound(kind, e_host):
    """1e-5 (output) / 2e-5 (gradient) are the project's bounds for a three-block stage against float64
    (tests/test_resblock_gpu.py::test_fused_stage_equals_fp64_autograd); the second term lets a tensor that fp32 itself cannot
    hold that tight -- conv_offset gradients, sums with cancellation -- scale with the fp32 evaluation's own error, by the ratio
    the project accepts between that bound and fp32 rounding: the device adds the same products in another order, in tiles and
    split partials, and the six-product split drops terms of relative size 2^-24."""
    return max({'out': 1e-5, 'grad': 2e-5}[kind], 16 * e_host)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Built once per case and never written: .layer (fp32, nudged parameters), .x, .go (the upstream gradient), .f64 and .f32
    (`evaluate` in either dtype on the host), .e_host = {tensor: deviation of .f32 from .f64}, .passes / .nudged."""
    layer, x, passes, nudged = build(name)
    with torch.no_grad():
        shape = stage_fp64(layer, x).shape
    go = torch.randn(shape, generator=torch.Generator().manual_seed(977 + list(CASES).index(name)))
    f64 = evaluate(copy.deepcopy(layer).double(), x.double(), go.double())
    f32 = evaluate(layer, x, go)
    e_host = {k: deviation(f32[k], f64[k]) for k in f64}
    return SimpleNamespace(name=name, layer=layer, x=x, go=go, f64=f64, f32=f32, e_host=e_host, passes=passes, nudged=nudged)


def compare(ref, got, keys=None):
    """[(tensor, error against float64, e_host, bound)] for the tensors in `got` ({'out' / 'x' / parameter name: tensor})."""
    rows = []
    for k in (got if keys is None else keys):
        rows.append((k, deviation(got[k], ref.f64[k]), ref.e_host[k], bound('out' if k == 'out' else 'grad', ref.e_host[k])))
    return rows


def report(tag, rows):
    """one line per tensor: error, e_host, their ratio, the share of the bound used"""
    for k, err, eh, bd in rows:
        print(f'STAGE {tag} {k}: err {err:.3e} e_host {eh:.3e} ratio {err / max(eh, 1e-300):.1f} of-bound {err / bd:.3f}')


def failures(rows):
    return [f'{k}: err {err:.3e} >= bound {bd:.3e} (e_host {eh:.3e}, ratio {err / max(eh, 1e-300):.1f})'
            for k, err, eh, bd in rows if not err < bd]
