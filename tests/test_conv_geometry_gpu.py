"""Dense convolution (ops/conv.py, csrc/conv.hip, csrc/conv_kernels.h, the weight-gradient routes of csrc/dcn.hip) on the
geometries of tests/conv_geometry_cases.py against fp64: rectangular taps, padding other than natural, even kernels and
strides beyond the kernel, dilation, one-pixel maps, batches that share a pixel tile, narrow channel counts, the row-merged
form, multi-level launches, the folded norm, and the geometries that stay with ATen.

Tolerances are those of tests/test_ops_gpu.py test_conv2d_matches_torch -- 3e-6 of the reference's range in 'bf16x6', 5e-5
in 'bf16x3' -- and of the tests this file extends (DENSE_TOL of tests/test_math_bf16_gpu.py, 5e-6 / 5e-4 for the folded norm).
With a ReLU the output gradient is zero wherever the fp64 pre-activation is within 1e-3 of the range of zero
(conv_geometry_cases.gate_safe), so every element is held by the maximum, gates included.  Each test prints its worst error
(`GEOM ...` lines, pytest -s)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import conv_geometry_cases as cg
from tests.test_math_bf16_gpu import DENSE_TOL, _check_dense
from tests.test_ops_gpu import _err

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
LSN_ERR_UNSUPPORTED = -2


def _dev():
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(params=['bf16x6', 'bf16x3'])
def split_mode(request):
    from lsnet_amd import _lib
    old = _lib.get_math_mode()
    _lib.set_math_mode(request.param)
    yield request.param
    _lib.set_math_mode(old)


def _tol(mode):
    return 3e-6 if mode == 'bf16x6' else 5e-5


def _cl(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


def _leaf(t):
    return None if t is None else _cl(t).requires_grad_() if t.dim() == 4 else t.to(_dev()).requires_grad_()


def _hold(what, got, want, tol):
    """every tensor of `got` within tol of the range of its reference; prints and returns the worst"""
    errs = {}
    for n, g, r in zip(('y', 'gx', 'gw', 'gb'), got, want):
        if r is None:
            continue
        assert g.shape == r.shape, (what, n, g.shape, r.shape)
        errs[n] = _err(g.double(), r)
    print(f'GEOM {what} ' + ' '.join(f'{n} {e:.2e}' for n, e in errs.items()))
    for n, e in errs.items():
        assert e < tol, (what, n, e)
    return max(errs.values())


def _run_conv2d(c, relu):
    """conv2d forward and every gradient on the device, under the case's shared inputs -> [y, gx, gw, gb]"""
    from lsnet_amd.ops.conv import conv2d
    x, w, b, go, _ = cg.reference(c, relu)
    xd, wd, bd = _leaf(x), _leaf(w), _leaf(b)
    y = conv2d(xd, wd, bd, c.s, c.p, c.d, relu=relu)
    assert y.is_contiguous(memory_format=_CL) and tuple(y.shape) == cg.out_shape(c)
    grads = torch.autograd.grad(y, [xd, wd] + ([bd] if bd is not None else []), _cl(go))
    return [y.detach()] + list(grads) + ([None] if bd is None else [])


# ---------------------------------------------------------------------------------- generic path: groups 1 .. 7
@pytest.mark.parametrize('c', cg.GENERIC, ids=[cg.case_id(c) for c in cg.GENERIC])
def test_conv2d_geometry_matches_fp64(c, split_mode):
    """Forward, data gradient, weight and bias gradient through `conv2d`, plain and with the ReLU epilogue."""
    for relu in (False, True):
        want = cg.reference(c, relu)[4]
        _hold(f'group {c.group} {split_mode} {cg.case_id(c)} relu {int(relu)}', _run_conv2d(c, relu), want, _tol(split_mode))


# ---------------------------------------------------------------------------------- single-product mode
def _pick(cases, **kw):
    return next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))


BF16_CASES = [_pick(cg.RECT, kh=3, kw=5, s=2, p=1, Co=136), _pick(cg.RECT, kh=7, kw=1, s=1, p=0, Co=48),
              _pick(cg.PAD, kh=3, s=1, p=0, Co=24),      # a 3x3 with Co <= 32: conv_np() == 1 hands the weight gradient over
              _pick(cg.PAD, kh=1, s=2, p=2, Co=256), _pick(cg.EVEN, kh=4, s=2, p=1, Co=48), _pick(cg.EVEN, kh=3, s=4, Co=136),
              _pick(cg.DIL, kh=5, s=2, d=2, Co=256), _pick(cg.DIL, kh=3, p=3, d=3, Co=24)]


@pytest.mark.parametrize('c', BF16_CASES, ids=[cg.case_id(c) for c in BF16_CASES])
def test_conv2d_geometry_bf16_matches_rounded_fp64(c):
    """'bf16': one product of the rounded operands -- equal to the fp64 convolution of the ROUNDED operands up to fp32
    summation, and away from the unrounded one (the one-product kernels ran)."""
    from lsnet_amd import _lib
    from lsnet_amd.ops.conv import conv2d
    assert c.group in (1, 2, 3, 4)
    x, w, b, go = cg.inputs(c)
    xd, wd, god = _leaf(x), _leaf(w), _cl(go)
    before = _lib.get_math_mode()
    try:
        _lib.set_math_mode('bf16')
        y = conv2d(xd, wd, None, c.s, c.p, c.d)
        gx, gw = torch.autograd.grad(y, [xd, wd], god)
    finally:
        _lib.set_math_mode(before)
    _check_dense(cg.case_id(c), [y, gx, gw], xd, wd, god, c.s, c.p, c.d, tol=DENSE_TOL)


# ---------------------------------------------------------------------------------- module path
MODULE_CASES = [_pick(cg.RECT, kh=3, kw=5, s=2, p=1, Co=48), _pick(cg.RECT, kh=1, kw=7, s=1, p=0, Co=256),
                _pick(cg.PAD, kh=3, s=1, p=3, Co=136), _pick(cg.EVEN, kh=4, s=4, Co=24), _pick(cg.DIL, kh=3, p=3, d=3, Co=48),
                _pick(cg.BATCH, B=8, kh=3, Co=24), _pick(cg.CHAN, C=8, Co=3, kh=3)]


@pytest.mark.parametrize('c', MODULE_CASES, ids=[cg.case_id(c) for c in MODULE_CASES])
def test_conv2d_module_geometry(c, split_mode):
    """A Conv2d module of the geometry, fed a channels-last and a contiguous (NCHW) input: channels-last results, the bits of
    the `conv2d` call (the same kernels in the same order), and with them fp64."""
    from lsnet_amd.ops.conv import Conv2d, hip_conv_ok
    x, w, b, go, want = cg.reference(c)
    base = _run_conv2d(c, False)
    _hold(f'module {split_mode} {cg.case_id(c)}', base, want, _tol(split_mode))
    for layout in ('nhwc', 'nchw'):
        m = Conv2d(c.C, c.Co, (c.kh, c.kw), stride=c.s, padding=c.p, dilation=c.d, bias=c.bias).to(_dev())
        with torch.no_grad():
            m.weight.copy_(w)
            if c.bias:
                m.bias.copy_(b)
        xd = x.to(_dev())
        if layout == 'nhwc':
            m, xd = m.to(memory_format=_CL), xd.contiguous(memory_format=_CL)
        xd.requires_grad_()
        assert hip_conv_ok(xd, m.weight, m.stride, m.padding, m.dilation, m.groups, m.padding_mode)
        y = m(xd)
        assert y.is_contiguous(memory_format=_CL)
        params = [m.weight] + ([m.bias] if c.bias else [])
        got = [y.detach()] + list(torch.autograd.grad(y, [xd] + params, go.to(_dev())))
        for n, g, r in zip(('y', 'gx', 'gw', 'gb'), got, base):
            assert torch.equal(g, r), (layout, n, _err(g, r.cpu()))


# ---------------------------------------------------------------------------------- row-merged form: group 8
class _Spy:
    """counts the calls of a function of ops/conv.py"""

    def __init__(self, monkeypatch, name):
        import lsnet_amd.ops.conv as conv
        self.calls = 0
        inner = getattr(conv, name)

        def wrapped(*a, **kw):
            self.calls += 1
            return inner(*a, **kw)
        monkeypatch.setattr(conv, name, wrapped)


@pytest.mark.parametrize('c,relu', cg.ROW_MERGED, ids=[cg.case_id(c) + f'-relu{int(r)}' for c, r in cg.ROW_MERGED])
def test_row_merged_forward_geometry(c, relu, split_mode, monkeypatch):
    """C < 8, kw > 1, no gradient: `conv2d` takes _stem_forward (the padded image, kw x C4 floats of a tap row as one channel
    run).  The same convolution with gradients takes the generic path on zero-padded channels.  Both against fp64."""
    from lsnet_amd.ops.conv import conv2d
    spy = _Spy(monkeypatch, '_stem_forward')
    x, w, b, go, want = cg.reference(c, relu)
    with torch.no_grad():
        y = conv2d(_cl(x), _cl(w), None if b is None else b.to(_dev()), c.s, c.p, c.d, relu=relu)
    assert spy.calls == 1 and y.is_contiguous(memory_format=_CL)
    _hold(f'group 8 {split_mode} {cg.case_id(c)} relu {int(relu)} row-merged', [y], want[:1], _tol(split_mode))
    got = _run_conv2d(c, relu)
    assert spy.calls == 1
    _hold(f'group 8 {split_mode} {cg.case_id(c)} relu {int(relu)} with-grad', got, want, _tol(split_mode))


# ---------------------------------------------------------------------------------- multi-level launches
# name: (C, Co, (kh, kw), pad, bias, relu, residuals, level sizes)
_L5 = [(13, 21), (7, 11), (4, 6), (1, 1), (2, 3)]
MULTI_CASES = {
    '1x3_p1_64_27': (64, 27, (1, 3), 1, True, False, False, _L5),                        # Co8 padding in conv_multi_dgrad, a 1 x 1 level
    '3x3_p0_32_2': (32, 2, (3, 3), 0, True, False, False, [(13, 21), (7, 11), (4, 6), (3, 3)]),
    '3x3_p0_64_27': (64, 27, (3, 3), 0, False, False, False, [(13, 21), (7, 11), (3, 5)]),
    '1x3_p1_32_2_relu': (32, 2, (1, 3), 1, False, True, False, _L5),
    '3x3_p1_64_27_relu_8_levels': (64, 27, (3, 3), 1, True, True, False, _L5 + [(9, 11), (5, 7), (3, 3)]),
    '1x3_p1_32_2_9_levels': (32, 2, (1, 3), 1, True, False, False, _L5 + [(9, 11), (5, 7), (3, 3), (6, 5)]),
    '1x3_p1_32_24_residuals': (32, 24, (1, 3), 1, True, False, True, _L5),
    '3x3_p0_64_48_residuals_relu': (64, 48, (3, 3), 0, True, True, True, [(13, 21), (7, 11), (4, 6), (3, 3)]),
}


@pytest.mark.parametrize('name', list(MULTI_CASES))
def test_conv2d_multi_level_geometry(name, split_mode, monkeypatch):
    """Conv2d.forward_multi == level-by-level calls == fp64: outputs, input gradients, the summed weight / bias gradient and
    the residuals' gradients.  Up to 8 levels are ONE launch per pass (conv2d_multi), nine are per-level calls."""
    from lsnet_amd.ops.conv import Conv2d
    C, Co, k, pad, bias, relu, res, sizes = MULTI_CASES[name]
    spy = _Spy(monkeypatch, 'conv2d_multi')
    tol = _tol(split_mode)
    g = torch.Generator().manual_seed(60 + len(name))
    m = Conv2d(C, Co, k, padding=pad, bias=bias).to(_dev()).to(memory_format=_CL)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (C * k[0] * k[1]) ** 0.5)
        if bias:
            m.bias.copy_(torch.randn(Co, generator=g))
    B = 2
    xs = [torch.randn(B, C, h, w, generator=g) for h, w in sizes]
    osz = [(h + 2 * pad - k[0] + 1, w + 2 * pad - k[1] + 1) for h, w in sizes]
    rs = [torch.randn(B, Co, h, w, generator=g) for h, w in osz] if res else []
    gos = [torch.randn(B, Co, h, w, generator=g) for h, w in osz]
    # fp64
    d = lambda t: t.detach().double().cpu()
    xr, rr = [d(x).requires_grad_() for x in xs], [d(r).requires_grad_() for r in rs]
    pr = [d(p).contiguous().requires_grad_() for p in m.parameters()]
    yr = [F.conv2d(x, pr[0], pr[1] if bias else None, 1, pad) for x in xr]
    yr = [y + r for y, r in zip(yr, rr)] if res else yr
    if relu:
        gos = [cg.gate_safe(y.detach(), go.double()).float() for y, go in zip(yr, gos)]
        yr = [F.relu(y) for y in yr]
    gr = torch.autograd.grad(yr, xr + rr + pr, [go.double() for go in gos])
    # the device, one launch per pass
    xd, rd, god = [_leaf(x) for x in xs], [_leaf(r) for r in rs], [_cl(go) for go in gos]
    params = list(m.parameters())
    outs = m.forward_multi(xd, relu=relu, residuals=rd if res else None)
    assert spy.calls == (1 if len(sizes) <= 8 else 0)
    g_multi = torch.autograd.grad(outs, xd + rd + params, god)
    # level by level
    singles = [m(x) for x in xd]
    singles = [y + r for y, r in zip(singles, rd)] if res else singles
    singles = [F.relu(y) for y in singles] if relu else singles
    g_single = torch.autograd.grad(singles, xd + rd + params, god)
    worst = 0.0
    for a, s_, r in zip(list(outs) + list(g_multi), list(singles) + list(g_single), [y.detach() for y in yr] + list(gr)):
        assert a.shape == r.shape
        e_single, e_ref = _err(a, s_.detach().cpu()), _err(a.double(), r)
        worst = max(worst, e_ref)
        assert e_single < tol and e_ref < tol and _err(s_.double(), r) < tol, (name, tuple(a.shape), e_single, e_ref)
    print(f'GEOM multi {split_mode} {name} worst {worst:.2e}')


# ---------------------------------------------------------------------------------- folded norm
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('k,s,p', [((1, 3), 1, 1), ((3, 3), 1, 0), ((2, 2), 2, 0), ((3, 3), 2, 2)])
def test_conv_bn_act_folded_geometry(k, s, p, res, relu, split_mode):
    """relu(bn(conv(x)) + residual) with the eval-mode norm folded into the weight image (ops/conv.py conv_bn_act), against the
    fp64 composition and at the tolerances of tests/test_ops_gpu.py test_conv_bn_act_folded, gamma = 0, 1e-6 and negative
    channels included."""
    from lsnet_amd.ops.conv import Conv2d, conv_bn_act
    torch.manual_seed(5)
    dev = _dev()
    tol = 5e-6 if split_mode == 'bf16x6' else 5e-4
    B, C, Co, H, W = 2, 32, 64, 19, 23
    conv = Conv2d(C, Co, k, stride=s, padding=p, bias=False).to(dev).to(memory_format=_CL)
    bn = torch.nn.BatchNorm2d(Co).to(dev).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Co) + 0.5)
        bn.weight[:4] = 0.0
        bn.weight[4:8] = 1e-6
        bn.weight[8:12] *= -1.0
        bn.bias.copy_(torch.randn(Co) * 0.3)
        bn.running_mean.copy_(torch.randn(Co) * 0.2)
        bn.running_var.copy_(torch.rand(Co) + 0.5)
    x = torch.randn(B, C, H, W, device=dev).contiguous(memory_format=_CL).requires_grad_()
    Ho, Wo = cg.out_size(H, k[0], s, p, 1), cg.out_size(W, k[1], s, p, 1)
    r = torch.randn(B, Co, Ho, Wo, device=dev).contiguous(memory_format=_CL).requires_grad_() if res else None
    go = torch.randn(B, Co, Ho, Wo, device=dev)
    d = lambda t: t.detach().double().cpu()
    xr, wr, gr, br = d(x).requires_grad_(), d(conv.weight).contiguous().requires_grad_(), d(bn.weight).requires_grad_(), \
        d(bn.bias).requires_grad_()
    rr = d(r).requires_grad_() if res else None
    z = F.batch_norm(F.conv2d(xr, wr, None, s, p), d(bn.running_mean), d(bn.running_var), gr, br, False, 0.0, bn.eps)
    if res:
        z = z + rr
    go = cg.gate_safe(z.detach(), d(go)) if relu else d(go)
    yr = F.relu(z) if relu else z
    gref = torch.autograd.grad(yr, [xr, wr, gr, br] + ([rr] if res else []), go)
    y = conv_bn_act(conv, bn, x, relu=relu, residual=r)
    assert y is not None and y.is_contiguous(memory_format=_CL)
    grads = torch.autograd.grad(y, [x, conv.weight, bn.weight, bn.bias] + ([r] if res else []), go.float().to(dev))
    errs = {'y': _err(y.double(), yr)}
    for g, ref, n in zip(grads, gref, ('gx', 'gw', 'ggamma', 'gbeta', 'gres')):
        errs[n] = _err(g.double(), ref)
    print(f'GEOM folded {split_mode} k {k} s {s} p {p} res {int(res)} relu {int(relu)} ' + ' '.join(f'{n} {e:.2e}' for n, e in errs.items()))
    for n, e in errs.items():
        assert e < tol, (n, e)


# ---------------------------------------------------------------------------------- geometries the kernels decline
DECLINED = {
    'same': dict(kernel_size=3, padding='same'),
    'reflect': dict(kernel_size=3, padding=1, padding_mode='reflect'),
    'stride_2_1': dict(kernel_size=3, stride=(2, 1), padding=1),
    'padding_1_0': dict(kernel_size=3, padding=(1, 0)),
    'dilation_1_2': dict(kernel_size=3, padding=2, dilation=(1, 2)),
    '9x9': dict(kernel_size=9, padding=4),
    'fp16': dict(kernel_size=3, padding=1),
}


@pytest.mark.parametrize('name', list(DECLINED))
def test_declined_geometry_comes_back_from_aten(name, monkeypatch):
    """What hip_conv_ok declines is ATen's convolution, announced by the fallback warning: equal to fp64 to 1e-5 of the range
    (fp16: to the precision of the type, 2^-10)."""
    import lsnet_amd.ops.conv as conv
    monkeypatch.setattr(conv, '_warned_fallbacks', set())
    kw = DECLINED[name]
    half = name == 'fp16'
    g = torch.Generator().manual_seed(31)
    m = conv.Conv2d(16, 24, **kw).to(_dev()).to(memory_format=_CL)
    x = torch.randn(3, 16, 13, 17, generator=g).to(_dev()).contiguous(memory_format=_CL)
    if half:
        m, x = m.half(), x.half()
    assert not conv.hip_conv_ok(x, m.weight, m.stride, m.padding, m.dilation, m.groups, m.padding_mode)
    with pytest.warns(RuntimeWarning, match='falling back to the ATen operator'):
        y = m(x)
    assert y.dtype == x.dtype
    ref = torch.nn.Conv2d(16, 24, **kw).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in m.state_dict().items()})
    e = _err(y.double(), ref(x.double().cpu()).detach())
    print(f'GEOM declined {name} {e:.2e}')
    assert e < (2.0 ** -10 if half else 1e-5), e


def test_more_than_64_taps_is_unsupported_at_the_c_entry():
    """A 9 x 9 kernel at the C ABI: LSN_ERR_UNSUPPORTED with the geometry in the message, from the prepared form, the one-shot
    form (which prepares the image first) and the image size query's companion lsn_conv2d_prepare_weights."""
    from lsnet_amd import _lib
    lib = _lib.load()
    dev = _dev()
    x = torch.randn(1, 16, 13, 17, device=dev).contiguous(memory_format=_CL)
    w = torch.randn(24, 16, 9, 9, device=dev).contiguous(memory_format=_CL)
    out = torch.empty(1, 24, 13, 17, device=dev).contiguous(memory_format=_CL)
    img = torch.empty(1 << 20, device=dev, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lv = (_lib.ConvLevel * 1)()
    lv[0].x, lv[0].out, lv[0].B, lv[0].H, lv[0].W = x.data_ptr(), out.data_ptr(), 1, 13, 17
    for call in (lambda: lib.lsn_conv2d_forward_prepared(1, lv, p(img), None, 16, 16, 24, 9, 9, 1, 4, 1, 0, None),
                 lambda: lib.lsn_conv2d_forward(p(x), p(w), None, p(out), None, 1, 13, 17, 16, 24, 9, 9, 1, 4, 1, 0, None),
                 lambda: lib.lsn_conv2d_prepare_weights(0, p(w), p(img), 16, 24, 9, 9, 1, 4, 1, None)):
        rc = call()
        assert rc == LSN_ERR_UNSUPPORTED and b'at most 64 taps, got 9 x 9' in lib.lsn_last_error(), (rc, lib.lsn_last_error())
    torch.cuda.synchronize()
