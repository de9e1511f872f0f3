"""The pooling family as kernels of the library (lsn_max_pool2d_* / lsn_avg_pool2d_* / lsn_upsample_add_* / lsn_corner_pool_*;
csrc/pool.hip) on the MI355X.  The reference is torch on the CPU throughout -- never the code under test, and not ATen on the
device, whose channels-last average-pool backward is wrong on this stack.

Exact cases: integer-valued gradients (and integer inputs for the average pool) make every sum exact in fp32, so forward and
backward are compared with torch.equal.  Real-valued cases: forwards of max pool, upsample-add and corner pool stay
torch.equal; where a result is a sum of n rounded terms the bound is |got - ref64| <= n * 2^-23 * S, with ref64 the float64
result on the CPU and S the same computation applied to the absolute values of the terms.  No outlier budget."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from lsnet_amd import _lib
from lsnet_amd.ops import conv as conv_ops
from lsnet_amd.ops import corner_pool as cp
from lsnet_amd.ops import pool
from lsnet_amd.ops.backend import get_backend
from tests import golden_cases as gc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CL = torch.channels_last
EPS = 2.0 ** -23
KINDS = ['int', 'real']
AVG_CFGS = [(3, 2, 1, False, True), (2, 2, 0, True, False)]
MAX_CASES = [((2, 64, 400, 672), 3, 2, 1), ((2, 64, 239, 335), 3, 2, 1), ((2, 256, 25, 42), 1, 2, 0), ((2, 256, 13, 21), 1, 2, 0)]
UP_CASES = [((25, 42), (50, 84)), ((50, 84), (100, 168)), ((13, 21), (25, 42)), ((25, 42), (50, 83)), ((25, 42), (49, 84))]
CORNER_SHAPES = [(2, 64, 100, 168), (2, 64, 50, 84), (2, 64, 25, 42), (2, 64, 13, 21), (2, 64, 7, 11), (2, 128, 25, 42)]
MODES = ['top', 'bottom', 'left', 'right']
POOL_OPS = ('max_pool2d', 'avg_pool2d', 'upsample_add', 'corner_pool')


def _be():
    return get_backend(torch.zeros(1, device=DEV))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed))


def _ints(seed, *shape):
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float()


def _relu_randn(seed, *shape):
    x = torch.relu(_randn(seed, *shape))
    assert (x == 0).float().mean() > 0.3, 'ties must really be present'
    return x


def _dev(t):
    """a host tensor as a dense channels-last device tensor"""
    return t.to(DEV).contiguous(memory_format=CL)


def _dev_slice(t, wide, start):
    """`t` (B, C, H, W) as the channel slice [start, start + C) of a dense channels-last device tensor with `wide` channels"""
    B, C, H, W = t.shape
    full = torch.full((B, wide, H, W), float('nan'), device=DEV).contiguous(memory_format=CL)
    full[:, start:start + C] = t.to(DEV)
    return full[:, start:start + C]


def _within(got, ref64, S, n, what):
    """|got - ref64| <= n * 2^-23 * S in every element; prints the worst ratio before it asserts"""
    err = (got.detach().cpu().double() - ref64).abs()
    bound = n * EPS * S.double()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: worst error {float(err.max()):.3e}, worst error / bound {ratio:.3f} (n = {n})')
    assert bool((err <= bound).all()), f'{what}: error beyond n * 2^-23 * S (worst ratio {ratio:.3f})'


def _grad_check(kind, got, ref_fn, go, n, what):
    """ref_fn(g) = the CPU gradient for an upstream gradient g (any dtype)"""
    if kind == 'int':
        assert torch.equal(got.cpu(), ref_fn(go)), what
    else:
        _within(got, ref_fn(go.double()), ref_fn(go.abs().double()), n, what)


@contextlib.contextmanager
def _watch(monkeypatch):
    """counts the calls of the backend's pooling methods and records the pooling family's ATen fall-backs"""
    be = _be()
    calls, fallbacks = {}, []
    with monkeypatch.context() as m:
        for name in ('max_pool2d_forward', 'max_pool2d_backward', 'avg_pool2d_forward', 'avg_pool2d_backward',
                     'upsample_add_forward', 'upsample_add_backward', 'corner_pool_forward', 'corner_pool_backward'):
            def wrapper(*a, _f=getattr(be, name), _n=name, **k):
                calls[_n] = calls.get(_n, 0) + 1
                return _f(*a, **k)
            m.setattr(be, name, wrapper, raising=False)
        warn = conv_ops._warn_aten_fallback

        def record(what, x, detail):
            if what in POOL_OPS and torch.is_tensor(x) and x.is_cuda:
                fallbacks.append((what, detail))
            return warn(what, x, detail)
        m.setattr(conv_ops, '_warn_aten_fallback', record)
        yield calls, fallbacks


def _off(monkeypatch, fn):
    with monkeypatch.context() as m:
        m.setattr(pool, 'NATIVE_POOL', False)
        return fn()


# ---- 1, 2: entry points and functions against the CPU ----------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape,k,s,p', MAX_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_max_pool(monkeypatch, kind, shape, k, s, p):
    x = (_relu_randn(1, *shape) if kind == 'int' else _randn(1, *shape)).requires_grad_()
    want = F.max_pool2d(x, k, s, p)
    go = _ints(2, *want.shape) if kind == 'int' else _randn(2, *want.shape)
    x64 = x.detach().double().requires_grad_()
    want64 = F.max_pool2d(x64, k, s, p)

    def ref(g):
        src, out = (x, want) if g.dtype == torch.float32 else (x64, want64)
        return torch.autograd.grad(out, src, g, retain_graph=True)[0]
    be = _be()
    xd = _dev(x.detach())
    y, slot = be.max_pool2d_forward(xd, (k, k), s, p, want_slot=k > 1)
    assert torch.equal(y.cpu(), want.detach()) and y.is_contiguous(memory_format=CL)
    gx = be.max_pool2d_backward(_dev(go), slot, tuple(shape), (k, k), s, p)
    _grad_check(kind, gx, ref, go, 4, f'max pool {k}/{s}/{p} {shape} backward (entry point)')
    with _watch(monkeypatch) as (calls, fallbacks):
        xa = xd.clone().requires_grad_()
        ya = pool.max_pool2d(xa, k, s, p)
        (ga,) = torch.autograd.grad(ya, xa, _dev(go))
    assert calls == {'max_pool2d_forward': 1, 'max_pool2d_backward': 1} and not fallbacks
    assert torch.equal(ya.detach().cpu(), want.detach()) and torch.equal(ga, gx)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cfg', AVG_CFGS, ids=['3-2-1', '2-2-0-ceil'])
@pytest.mark.parametrize('shape,wide,start', [((2, 208, 13, 17), 832, 624), ((2, 104, 25, 42), 416, 312), ((2, 256, 25, 42), 256, 0)],
                         ids=['832x13x17_slice', '416x25x42_slice', '256x25x42_dense'])
def test_avg_pool(monkeypatch, kind, cfg, shape, wide, start):
    k, s, p, ceil_mode, cip = cfg
    x = (_ints(3, *shape) if kind == 'int' else _randn(3, *shape)).requires_grad_()
    want = F.avg_pool2d(x, k, s, p, ceil_mode, cip)
    go = _ints(4, *want.shape) if kind == 'int' else _randn(4, *want.shape)
    x64 = x.detach().double().requires_grad_()
    want64 = F.avg_pool2d(x64, k, s, p, ceil_mode, cip)

    def ref(g):
        src, out = (x, want) if g.dtype == torch.float32 else (x64, want64)
        return torch.autograd.grad(out, src, g, retain_graph=True)[0]
    be = _be()
    xd = _dev_slice(x.detach(), wide, start)
    assert (wide == shape[1]) == xd.is_contiguous(memory_format=CL)
    y = be.avg_pool2d_forward(xd, (k, k), s, p, ceil_mode, cip)
    assert y.shape == want.shape
    if kind == 'int':
        assert torch.equal(y.cpu(), want.detach())
    else:
        _within(y, want64.detach(), F.avg_pool2d(x.detach().abs().double(), k, s, p, ceil_mode, cip), k * k,
                f'avg pool {cfg} {shape} forward')
    gx = be.avg_pool2d_backward(_dev(go), tuple(shape), (k, k), s, p, ceil_mode, cip)
    _grad_check(kind, gx, ref, go, 4, f'avg pool {cfg} {shape} backward (entry point)')
    with _watch(monkeypatch) as (calls, fallbacks):
        full = xd._base.detach().clone().requires_grad_() if xd._base is not None else xd.detach().clone().requires_grad_()
        xa = full[:, start:start + shape[1]]
        ya = pool.avg_pool2d(xa, k, s, p, ceil_mode, cip)
        (gfull,) = torch.autograd.grad(ya, full, _dev(go))
    assert calls == {'avg_pool2d_forward': 1, 'avg_pool2d_backward': 1} and not fallbacks
    assert torch.equal(ya.detach(), y) and torch.equal(gfull[:, start:start + shape[1]], gx)
    assert wide == shape[1] or not bool(gfull[:, :start].any())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw,HW', UP_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_upsample_add(monkeypatch, kind, hw, HW):
    make = _ints if kind == 'int' else _randn
    top, lat, go = make(5, 2, 256, *hw).requires_grad_(), make(6, 2, 256, *HW).requires_grad_(), make(7, 2, 256, *HW)
    want = lat + F.interpolate(top, size=HW, mode='nearest')

    def ref(g):
        t = top.detach().to(g.dtype).requires_grad_()
        return torch.autograd.grad(F.interpolate(t, size=HW, mode='nearest'), t, g)[0]
    be = _be()
    td, ld, gd = _dev(top.detach()), _dev(lat.detach()), _dev(go)
    out = be.upsample_add_forward(td, ld)
    assert torch.equal(out.cpu(), want.detach())
    inplace = ld.clone()
    assert be.upsample_add_forward(td, inplace, out=inplace) is inplace and torch.equal(inplace, out)
    gt = be.upsample_add_backward(gd, tuple(top.shape))
    _grad_check(kind, gt, ref, go, 4, f'upsample-add {hw} -> {HW} backward')
    if kind == 'int':
        base = _dev(_ints(8, *top.shape))
        acc = be.upsample_add_backward(gd, tuple(top.shape), out=base.clone(), accumulate=True)
        assert torch.equal(acc, base + gt)
    with _watch(monkeypatch) as (calls, fallbacks):
        ta, la = td.clone().requires_grad_(), ld.clone().requires_grad_()
        oa = pool.upsample_add(ta, la)
        g_top, g_lat = torch.autograd.grad(oa, [ta, la], gd)
    assert calls == {'upsample_add_forward': 1, 'upsample_add_backward': 1} and not fallbacks
    assert torch.equal(oa.detach(), out) and torch.equal(g_top, gt) and torch.equal(g_lat, gd)


def _cummax_pool(x, mode):
    dim, flip = cp.CornerPool.DIM_FLIP[mode]
    if flip:
        x = x.flip(dim)
    out = torch.cummax(x, dim=dim)[0]
    return out.flip(dim) if flip else out


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', CORNER_SHAPES, ids=lambda v: 'x'.join(map(str, v)))
def test_corner_pool(monkeypatch, kind, shape):
    be = _be()
    x = _relu_randn(9, *shape) if kind == 'int' else _randn(9, *shape)
    go = _ints(10, *shape) if kind == 'int' else _randn(10, *shape)
    xd, gd = _dev(x), _dev(go)
    base_y, base_g = _dev(_ints(11, *shape)), _dev(_ints(12, *shape))
    for mode in MODES:
        want = _cummax_pool(x, mode)

        def ref(g):
            t = x.to(g.dtype).requires_grad_()
            return torch.autograd.grad(_cummax_pool(t, mode), t, g)[0]
        n = shape[3] if mode in ('left', 'right') else shape[2]
        y = be.corner_pool_forward(mode, xd)
        assert torch.equal(y.cpu(), want), mode
        gx = be.corner_pool_backward(mode, xd, gd)
        _grad_check(kind, gx, ref, go, n, f'corner pool {mode} {shape} backward')
        if kind == 'int':       # accumulate on: integer sums stay exact
            ya = be.corner_pool_forward(mode, xd.round(), out=base_y.clone(), accumulate=True)
            assert torch.equal(ya.cpu(), base_y.cpu() + _cummax_pool(x.round(), mode)), mode
            ga = be.corner_pool_backward(mode, xd, gd, out=base_g.clone(), accumulate=True)
            assert torch.equal(ga, base_g + gx), mode
        else:                   # accumulate on: one more rounded add per element
            ya = be.corner_pool_forward(mode, xd, out=y.clone(), accumulate=True)
            assert torch.equal(ya, y + y), mode
            ga = be.corner_pool_backward(mode, xd, gd, out=gx.clone(), accumulate=True)
            assert torch.equal(ga, gx + gx), mode
        with _watch(monkeypatch) as (calls, fallbacks):
            xa = xd.clone().requires_grad_()
            ym = cp.CornerPool(mode)(xa)
            (gm,) = torch.autograd.grad(ym, xa, gd)
        assert calls == {'corner_pool_forward': 1, 'corner_pool_backward': 1} and not fallbacks
        assert torch.equal(ym.detach(), y) and torch.equal(gm, gx), mode
    # the pooling blocks' sum of two pools: two launches, no add
    for m1, m2 in (('top', 'left'), ('bottom', 'right')):
        x2 = _relu_randn(13, *shape) if kind == 'int' else _randn(13, *shape)
        with _watch(monkeypatch) as (calls, fallbacks):
            a, b = xd.clone().requires_grad_(), _dev(x2).requires_grad_()
            s = cp.corner_pool_sum(a, m1, b, m2)
            ga, gb = torch.autograd.grad(s, [a, b], gd)
        assert calls == {'corner_pool_forward': 2, 'corner_pool_backward': 2} and not fallbacks
        assert torch.equal(s.detach().cpu(), _cummax_pool(x, m1) + _cummax_pool(x2, m2))
        assert torch.equal(ga, be.corner_pool_backward(m1, xd, gd)) and torch.equal(gb, be.corner_pool_backward(m2, _dev(x2), gd))


@pytest.mark.parametrize('special', ['inf', 'nan'])
def test_inf_and_nan(special):
    be = _be()
    x = _relu_randn(14, 2, 8, 13, 21)
    v = float(special)
    x[0, 0, 6, 10], x[0, 0, 6, 15], x[0, 0, 2, 10], x[1, 2, 0, 0], x[1, 1, 12, 20] = v, v, v, v, v
    x[1, 3, :5, :5] = float('-inf')
    go = _ints(15, 2, 8, 13, 21)

    def same(a, b):
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    xd = _dev(x)
    for mode in MODES:
        t = x.clone().requires_grad_()
        want = _cummax_pool(t, mode)
        (gwant,) = torch.autograd.grad(want, t, go)
        assert same(be.corner_pool_forward(mode, xd).cpu(), want.detach()), mode
        assert torch.equal(be.corner_pool_backward(mode, xd, _dev(go)).cpu(), gwant), mode
    t = x.clone().requires_grad_()
    want = F.max_pool2d(t, 3, 2, 1)
    g2 = _ints(16, *want.shape)
    (gwant,) = torch.autograd.grad(want, t, g2)
    y, slot = be.max_pool2d_forward(xd, (3, 3), 2, 1)
    assert same(y.cpu(), want.detach()) and bool(torch.isnan(y).any()) == (special == 'nan')
    assert torch.equal(be.max_pool2d_backward(_dev(g2), slot, tuple(x.shape), (3, 3), 2, 1).cpu(), gwant)


# ---- 3: the case ATen's channels-last kernel gets wrong ------------------------------------------------------------------
@pytest.mark.parametrize('sliced', [True, False], ids=['slice', 'dense'])
@pytest.mark.parametrize('k,s,p,ceil,cip', AVG_CFGS)
def test_avg_pool_defect_case(monkeypatch, k, s, p, ceil, cip, sliced):
    """The inputs of tests/test_ops_gpu.py::test_avg_pool_backward through the native path, on the channels-last slice (and on
    a dense channels-last copy of it): the gradient ATen's channels-last kernel returns off by 0.68 of its range."""
    torch.manual_seed(0)
    x = torch.randn(2, 832, 13, 17)
    xs = x[:, 624:].double().requires_grad_()
    yh = F.avg_pool2d(xs, k, s, p, ceil, cip)
    go = torch.randn(yh.shape, dtype=torch.float32)
    ref = torch.autograd.grad(yh, xs, go.double(), retain_graph=True)[0]
    S = torch.autograd.grad(yh, xs, go.abs().double())[0]
    with _watch(monkeypatch) as (calls, fallbacks):
        xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_()
        src = xd[:, 624:] if sliced else xd[:, 624:].contiguous(memory_format=CL)
        yd = pool.avg_pool(src, torch.nn.AvgPool2d(k, s, p, ceil_mode=ceil, count_include_pad=cip))
        yd.backward(go.to(DEV).contiguous(memory_format=CL))
    assert calls == {'avg_pool2d_forward': 1, 'avg_pool2d_backward': 1} and not fallbacks
    _within(yd, yh.detach(), F.avg_pool2d(x[:, 624:].abs().double(), k, s, p, ceil, cip), k * k, 'forward')
    _within(xd.grad[:, 624:], ref, S, 4, f'avg pool {(k, s, p, ceil, cip)} gradient, {"slice" if sliced else "dense"}')
    assert not bool(xd.grad[:, :624].any())


# ---- 4: modules, switch on against switch off ------------------------------------------------------------------------------
def _close(a, b, what):
    scale = max(float(b.abs().max()), 1e-12)
    worst = float((a - b).abs().max()) / scale
    print(f'{what}: off by {worst:.3e} of the range')
    assert worst <= gc.FP_TOL, (what, worst)


def _run_module(fn_forward, params, inputs):
    outs = fn_forward()
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    proj = sum((o * torch.randn(o.shape, generator=_gen(70 + i)).to(DEV)).sum() / o.numel() ** 0.5 for i, o in enumerate(outs))
    grads = torch.autograd.grad(proj, inputs + params)      # (every one of them takes part: an unused one is an error)
    return [o.detach() for o in outs], grads


def _on_against_off(monkeypatch, forward, params, inputs, expect_calls, what):
    with _watch(monkeypatch) as (calls, fallbacks):
        outs, grads = _run_module(forward, params, inputs)
    assert not fallbacks, fallbacks
    for name, count in expect_calls.items():
        assert calls.get(name, 0) == count, (what, name, calls)
    with _watch(monkeypatch) as (calls_off, _):
        outs_off, grads_off = _off(monkeypatch, lambda: _run_module(forward, params, inputs))
    assert not calls_off
    for i, (a, b) in enumerate(zip(outs, outs_off)):
        assert torch.equal(a, b), f'{what}: output {i}'
    for i, (a, b) in enumerate(zip(grads, grads_off)):
        _close(a, b, f'{what}: gradient {i}')


@pytest.mark.parametrize('hw', [(256, 320), (239, 335)], ids=['256x320', '239x335'])
def test_resnet50_fpn_on_against_off(monkeypatch, hw):
    from lsnet_amd.models import build_backbone, build_neck
    bb = build_backbone(dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                             norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch'))
    neck = build_neck(dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
                           add_extra_convs='on_input', num_outs=5, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)))
    gu.fill_params(bb, seed=3); gu.fill_params(neck, seed=4)
    bb, neck = bb.to(DEV).train().to(memory_format=CL), neck.to(DEV).train().to(memory_format=CL)
    x = _dev(_randn(21, 2, 3, *hw)).requires_grad_()
    params = [p for p in list(bb.parameters()) + list(neck.parameters()) if p.requires_grad]
    _on_against_off(monkeypatch, lambda: neck(bb(x)), params, [x],
                    dict(max_pool2d_forward=1, max_pool2d_backward=1, upsample_add_forward=2, upsample_add_backward=2),
                    f'ResNet-50 + FPN {hw}')


def test_fpn_pooled_extra_levels_on_against_off(monkeypatch):
    from lsnet_amd.models import build_neck
    neck = build_neck(dict(type='FPN', in_channels=[256, 512, 1024], out_channels=256, num_outs=5))
    gu.fill_params(neck, seed=5)
    neck = neck.to(DEV).train().to(memory_format=CL)
    xs = [_dev(_randn(22 + i, 2, c, *s)).requires_grad_() for i, (c, s) in enumerate(((256, (50, 83)), (512, (25, 42)), (1024, (13, 21))))]
    _on_against_off(monkeypatch, lambda: neck(xs), list(neck.parameters()), xs,
                    dict(max_pool2d_forward=2, max_pool2d_backward=2, upsample_add_forward=2, upsample_add_backward=2),
                    'FPN with pooled extra levels')


def test_res2net_stage_on_against_off(monkeypatch):
    from lsnet_amd.models import build_backbone
    bb = build_backbone(dict(type='Res2Net', depth=50, scales=4, base_width=26, num_stages=4, out_indices=(0, 1, 2, 3),
                             frozen_stages=-1, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True))
    gu.fill_params(bb, seed=8)
    block = bb.layer2[0].to(DEV).train().to(memory_format=CL)        # stage_type 'stage', stride 2, avg_down shortcut
    assert block.stage_type == 'stage' and hasattr(block, 'pool') and isinstance(block.downsample[0], torch.nn.AvgPool2d)
    for m in block.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    x = _dev(_randn(23, 2, 256, 25, 42)).requires_grad_()
    _on_against_off(monkeypatch, lambda: block(x), [p for p in block.parameters() if p.requires_grad], [x],
                    dict(avg_pool2d_forward=2, avg_pool2d_backward=2), 'Bottle2neck stage block')


@pytest.mark.parametrize('corner_dim', [64, 128])
@pytest.mark.parametrize('cls', ['TLPool', 'BRPool'])
def test_corner_pool_blocks_on_against_off(monkeypatch, cls, corner_dim):
    block = getattr(cp, cls)(64, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), corner_dim=corner_dim)
    gu.fill_params(block, seed=9)
    block = block.to(DEV).train().to(memory_format=CL)
    x = _dev(_randn(24, 2, 64, 25, 42)).requires_grad_()
    _on_against_off(monkeypatch, lambda: block(x), list(block.parameters()), [x],
                    dict(corner_pool_forward=2, corner_pool_backward=2), f'{cls} corner_dim {corner_dim}')


# ---- 5: determinism -----------------------------------------------------------------------------------------------------
def test_backwards_are_bit_reproducible():
    be = _be()
    g_stem, x_stem = _dev(_randn(30, 2, 64, 200, 336)), _dev(_relu_randn(31, 2, 64, 400, 672))
    _, slot = be.max_pool2d_forward(x_stem, (3, 3), 2, 1)
    g_avg = _dev(_randn(32, 2, 104, 13, 21))
    g_up = _dev(_randn(33, 2, 256, 50, 83))
    x_c, g_c = _dev(_relu_randn(34, 2, 64, 100, 168)), _dev(_randn(35, 2, 64, 100, 168))
    runs = [lambda: be.max_pool2d_backward(g_stem, slot, (2, 64, 400, 672), (3, 3), 2, 1),
            lambda: be.max_pool2d_backward(g_avg, None, (2, 104, 25, 42), (1, 1), 2, 0),
            lambda: be.avg_pool2d_backward(g_avg, (2, 104, 25, 42), (3, 3), 2, 1, False, True),
            lambda: be.avg_pool2d_backward(g_avg, (2, 104, 25, 42), (2, 2), 2, 0, True, False),
            lambda: be.upsample_add_backward(g_up, (2, 256, 25, 42))] + \
           [lambda m=m: be.corner_pool_backward(m, x_c, g_c) for m in MODES]
    for i, run in enumerate(runs):
        assert torch.equal(run(), run()), i


def test_corner_pool_pack_parameter_gradients_are_bit_reproducible():
    """forward + backward of a pooling block twice: every parameter gradient the same bits (ATen's scatter_add backward of
    cummax adds with fp32 atomics and does not give this)."""
    block = cp.TLPool(64, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), corner_dim=128)
    gu.fill_params(block, seed=10)
    block = block.to(DEV).train().to(memory_format=CL)
    x = _dev(_randn(36, 2, 64, 100, 168)).requires_grad_()
    go = _dev(_randn(37, 2, 64, 100, 168))

    def run():
        return torch.autograd.grad(block(x), [x] + list(block.parameters()), go)
    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


# ---- 6: the rules of the training step -----------------------------------------------------------------------------------
def _step_ops():
    """(name, run) for every entry point, on preallocated tensors: run() writes into its own output and returns it"""
    be = _be()
    x = _dev(_relu_randn(40, 2, 64, 50, 84))
    wide = _dev(_randn(41, 2, 128, 50, 84))
    xs = wide[:, 64:]
    y_max, g_in = _dev(torch.zeros(2, 64, 25, 42)), _dev(torch.zeros(2, 64, 50, 84))
    _, slot = be.max_pool2d_forward(x, (3, 3), 2, 1)
    gy = _dev(_randn(42, 2, 64, 25, 42))
    top, up_out, g_top = _dev(_randn(43, 2, 64, 25, 42)), _dev(torch.zeros(2, 64, 50, 84)), _dev(torch.zeros(2, 64, 25, 42))
    c_out, c_grad = _dev(torch.zeros(2, 64, 50, 84)), _dev(torch.zeros(2, 64, 50, 84))
    ops = [('max_pool2d_forward', lambda: be.max_pool2d_forward(x, (3, 3), 2, 1, want_slot=False, out=y_max)[0]),
           ('max_pool2d_backward', lambda: be.max_pool2d_backward(gy, slot, (2, 64, 50, 84), (3, 3), 2, 1, out=g_in)),
           ('avg_pool2d_forward', lambda: be.avg_pool2d_forward(xs, (3, 3), 2, 1, False, True, out=y_max)),
           ('avg_pool2d_backward', lambda: be.avg_pool2d_backward(gy, (2, 64, 50, 84), (2, 2), 2, 0, True, False, out=g_in)),
           ('upsample_add_forward', lambda: be.upsample_add_forward(top, xs, out=up_out)),
           ('upsample_add_backward', lambda: be.upsample_add_backward(x, (2, 64, 25, 42), out=g_top))]
    for mode in MODES:
        ops.append((f'corner_pool_forward {mode}', lambda m=mode: be.corner_pool_forward(m, x, out=c_out)))
        ops.append((f'corner_pool_backward {mode}', lambda m=mode: be.corner_pool_backward(m, x, xs, out=c_grad)))
    return ops


def test_no_allocation_no_sync():
    ops = _step_ops()
    torch.cuda.synchronize()
    before = _lib.scratch_stats()
    for name, run in ops:
        run()
        torch.cuda.synchronize()
        assert _lib.scratch_stats() == before, name


def test_graph_capture_and_replay():
    """every op captured once into a single-stream graph; one replay gives the eager result"""
    ops = _step_ops()
    want = []
    for name, run in ops:
        want.append(run().clone())
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            for name, run in ops:
                outs.append(run())
                outs[-1] = outs[-1].clone()          # (several ops share an output buffer: keep each result inside the graph)
    torch.cuda.current_stream().wait_stream(stream)
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for (name, _), got, ref in zip(ops, outs, want):
        assert torch.equal(got, ref), name


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------
def test_refused_shapes_take_the_framework_statements(monkeypatch):
    be = _be()
    lib = _lib.load()
    x6 = _dev(_relu_randn(50, 2, 6, 13, 21))                                   # C % 4 != 0
    with pytest.raises(RuntimeError, match='not a multiple of 4'):
        be.max_pool2d_forward(x6, (3, 3), 2, 1)
    assert b'not a multiple of 4' in lib.lsn_last_error()
    x10 = _dev(_relu_randn(51, 2, 10, 13, 21))
    x8 = x10[:, :8]                                                            # pixel pitch 10 floats: rows not 16-byte aligned
    with pytest.raises(RuntimeError, match='pixel pitch of x is 10'):
        be.corner_pool_forward('top', x8)
    with pytest.raises(RuntimeError, match='pixel pitch of x is 10'):
        be.avg_pool2d_forward(x8, (3, 3), 2, 1, False, True)
    top, lat = _dev(_randn(52, 2, 8, 4, 4)), _dev(_randn(53, 2, 8, 9, 8))      # 9 is neither 2 * 4 nor 2 * 4 - 1
    with pytest.raises(RuntimeError, match='is not a doubling'):
        be.upsample_add_forward(top, lat)
    assert b'is not a doubling' in lib.lsn_last_error()
    with _watch(monkeypatch) as (calls, fallbacks):
        for t in (x6, x8):
            xa = t.detach().clone().requires_grad_() if t is x6 else x10.detach().clone().requires_grad_()
            src = xa if t is x6 else xa[:, :8]
            host = t.detach().cpu().contiguous().requires_grad_()
            go = _ints(54, 2, t.shape[1], 7, 11)
            for fn_dev, fn_host in ((lambda v: pool.max_pool2d(v, 3, 2, 1), lambda v: F.max_pool2d(v, 3, 2, 1)),
                                    (lambda v: pool.avg_pool2d(v, 3, 2, 1), lambda v: F.avg_pool2d(v, 3, 2, 1))):
                yd, yh = fn_dev(src), fn_host(host)
                (gd,), (gh,) = torch.autograd.grad(yd, xa, go.to(DEV)), torch.autograd.grad(yh, host, go)
                assert torch.allclose(yd.detach().cpu(), yh.detach(), rtol=1e-6, atol=1e-6)
                assert torch.allclose(gd.cpu()[:, :t.shape[1]], gh, rtol=1e-6, atol=1e-6)
            for mode in MODES:
                assert torch.equal(cp.CornerPool(mode)(src).detach().cpu(), _cummax_pool(host.detach(), mode))
        out = pool.upsample_add(top, lat)
        assert torch.equal(out.cpu(), lat.cpu() + F.interpolate(top.cpu(), size=(9, 8), mode='nearest'))
    assert not calls and {f[0] for f in fallbacks} == set(POOL_OPS)
