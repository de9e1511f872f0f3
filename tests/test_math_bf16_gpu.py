"""The single-product bf16 math mode ('bf16', LSN_MATH_BF16; include/lsnet_hip.h) on the device.

Arithmetic: every fp32 operand of a contraction is rounded to bf16 (round to nearest even) and each product is ONE bf16
MFMA with fp32 accumulation.  A product of two bf16 values is exact in fp32, so the kernels' results must equal a
convolution of the ROUNDED operands up to fp32 summation (checked against fp64), and must differ from the unrounded
result by the rounding (which proves that the one-product kernels ran).  Kernels without a split variant (grouped,
narrow and odd-channel deformable layers) keep their arithmetic in every mode."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import DCN_CASES, _dcn_all, _dcn_fp64, _err, _make

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'
    return torch.device('cuda:0')


def _bf(t):
    """round to nearest even bf16, back to the tensor's own type"""
    return t.float().to(torch.bfloat16).to(t.dtype)


@pytest.fixture
def math_mode():
    """set_math_mode(...) inside the test; the previous mode and debug word are restored afterwards"""
    from lsnet_amd import _lib
    before = _lib.get_math_mode()
    yield _lib.set_math_mode
    _lib.set_math_mode(before)
    _lib.set_debug_word(0)


# measured on the MI355X (bf16 against fp64 of the rounded operands, fraction of the output range): <= 2.9e-7 over the
# cases below, against 1.8e-3 .. 2.7e-3 from the unrounded operands
DENSE_TOL = 1e-6


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _check_dense(name, got, x, w, go, s, p, d, bias=None, residual=None, tol=DENSE_TOL):
    """got = [y, gx, gw] (gw may be None) against fp64 convolutions of the rounded and of the unrounded operands"""
    def ref(xr, wr, gr):
        xr = xr.detach().double().cpu().requires_grad_()
        wr = wr.detach().double().cpu().contiguous().requires_grad_()
        y = F.conv2d(xr, wr, None if bias is None else bias.detach().double().cpu(), s, p, d)
        if residual is not None:
            y = y + residual.detach().double().cpu()
        return [y.detach()] + list(torch.autograd.grad(y, [xr, wr], gr.detach().double().cpu()))
    rounded = ref(_bf(x), _bf(w), _bf(go))     # forward: x, w; data gradient: go, w; weight gradient: x, go
    exact = ref(x, w, go)
    for n, g, r, e in zip(('y', 'gx', 'gw'), got, rounded, exact):
        if g is None:
            continue
        er, ee = _err(g.double(), r), _err(g.double(), e)
        print(f'{name} {n}: vs rounded-operand fp64 {er:.2e}, vs unrounded fp64 {ee:.2e}')
        assert er <= tol, (name, n, er)
        assert ee > 1e-5, (name, n, ee)        # the one-product path ran (bf16x6 would be ~1e-7 here)


@pytest.mark.parametrize('B,C,Co,k,s,p,d,H,W', [
    (2, 256, 256, 3, 1, 1, 1, 50, 84), (2, 1024, 512, 1, 1, 0, 1, 25, 42),       # the shapes of test_conv_split6_matches_fp64
    (1, 2048, 256, 3, 2, 1, 1, 25, 42), (2, 128, 128, 3, 2, 1, 1, 40, 52),
    (2, 256, 27, 3, 1, 1, 1, 25, 42),                                             # the towers' offset / mask convolution
    (1, 512, 256, 3, 1, 1, 1, 64, 64),                                            # weight gradient on dcn_wgrad_mm_kernel<1, DENSE>
])
def test_conv_bf16_matches_rounded_fp64(B, C, Co, k, s, p, d, H, W, math_mode):
    from lsnet_amd.ops.conv import conv2d
    torch.manual_seed(7)
    dev = _dev()
    x = _cl(torch.randn(B, C, H, W, device=dev)).requires_grad_()
    w = _cl(torch.randn(Co, C, k, k, device=dev) / (C * k * k) ** 0.5).requires_grad_()
    math_mode('bf16')
    y = conv2d(x, w, None, s, p, d)
    go = _cl(torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)))
    gx, gw = torch.autograd.grad(y, [x, w], go)
    _check_dense((C, Co, k, s), [y, gx, gw], x, w, go, s, p, d)


def test_conv_bn_residual_epilogue_bf16(math_mode):
    """A folded-BatchNorm convolution with the residual in its epilogue (ops/conv.py conv_bn_act; the bottleneck's last
    convolution, ops/resblock.py): the image holds the SCALED weight, rounded.  Scales are powers of two (eps = 0), so the
    fold is exact and the rounded reference is bf16(w * scale)."""
    from lsnet_amd.ops.conv import Conv2d, conv_bn_act
    torch.manual_seed(5)
    dev = _dev()
    C, Co, B, H, W = 256, 512, 2, 19, 23
    conv = Conv2d(C, Co, 1, bias=False).to(dev).to(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(Co, eps=0.0).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (Co,), generator=g)])
        bn.running_var.copy_(torch.tensor([0.25, 1.0, 4.0])[torch.randint(0, 3, (Co,), generator=g)])
        bn.running_mean.copy_(torch.randn(Co, generator=g) * 0.2)
        bn.bias.copy_(torch.randn(Co, generator=g) * 0.3)
    x = _cl(torch.randn(B, C, H, W, device=dev)).requires_grad_()
    r = _cl(torch.randn(B, Co, H, W, device=dev)).requires_grad_()
    math_mode('bf16')
    y = conv_bn_act(conv, bn, x, relu=False, residual=r)
    assert y is not None
    go = torch.randn_like(y)
    gx, = torch.autograd.grad(y, [x], go)
    scale = (bn.weight / bn.running_var.sqrt()).detach()
    wf = conv.weight.detach() * scale.view(-1, 1, 1, 1)
    shift = (bn.bias - bn.running_mean * scale).detach()
    _check_dense('bn_residual', [y, gx], x, wf, go, 1, 0, 1, bias=shift, residual=r)


# ---------------------------------------------------------------------------------- deformable convolutions
_FP64 = {}
ROUNDED_FWD_FRAC = 3e-3   # 3x the measured worst share (1.04e-3, pyr_head: the pyramid's scaled positions)


def _truth(case, dev):
    if case['name'] not in _FP64:
        x, w, b, off, mask, go, cfg = _make(case, dev, seed=11)
        _FP64[case['name']] = _dcn_fp64(x, w, b, off, mask, go, cfg)
    return _FP64[case['name']]


def _rounded_forward(x, w, b, off, mask, cfg):
    """tests/torch_dcn_ref.py with the sampled, masked column and the weight rounded to bf16 before the product"""
    import tests.torch_dcn_ref as ref

    class _Torch:   # the module's `torch` with a rounding einsum
        def __getattr__(self, n):
            return getattr(torch, n)

        @staticmethod
        def einsum(eq, wm, col):
            return torch.einsum(eq, _bf(wm), _bf(col))
    saved = ref.torch
    ref.torch = _Torch()
    try:
        return ref.torch_dcn(x.double(), off.float(), None if mask is None else mask.double(), w.double(),
                             None if b is None else b.double(), cfg['stride'], cfg['pad'], cfg['dil'], cfg['groups'], cfg['dg'],
                             cfg['sh'], cfg['sw'])
    finally:
        ref.torch = saved


@pytest.mark.parametrize('routing', ['default', 'first_gemms'])
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('case', DCN_CASES, ids=[c['name'] for c in DCN_CASES])
def test_dcn_bf16(case, layout, routing, math_mode):
    """Every output and gradient within 1e-2 of the range of the fp64 evaluation.  An output whose kernels have a
    one-product form moves by the rounding (measured 1e-3 .. 4e-3 of its range, against the 'bf16x6' run as against fp64)
    and must be more than 1e-5 away from fp64; one that stays within 1e-5 of the 'bf16x6' run is computed by a kernel
    without a split variant (grouped layers, odd channel counts, the fp32 scatter kernels; their fp32 atomics make them
    differ in the last bits) and is held to 1e-4.  The wide single-group layers must run their contractions in bf16.  The
    forward, where it ran in bf16, equals the rounded-column evaluation to 1e-4 of its range but for isolated samples whose
    blended value lies at a bf16 rounding midpoint (the kernel's fp32 blend and the reference's differ in the last bit, so
    the two round apart by one bf16 step).  routing 'first_gemms': DBG_GENERAL_GEMMS, the GEMMs of dcn_kernels.h where
    dcn_mm_kernels.h would serve."""
    from lsnet_amd import _lib, ops
    dev = _dev()
    x, w, b, off, mask, go, cfg = _make(case, dev, seed=11)
    truth = _truth(case, dev)
    _lib.set_debug_word(_lib.DBG_GENERAL_GEMMS if routing == 'first_gemms' else 0)
    cl = layout == 'nhwc'
    math_mode('bf16x6')
    x6 = _dcn_all(ops, x, w, b, off, mask, go, cfg, dev, cl)
    math_mode('bf16')
    got = _dcn_all(ops, x, w, b, off, mask, go, cfg, dev, cl)
    split = {k: _err(got[k], x6[k]) > 1e-5 for k in truth}
    err = {k: _err(got[k].double(), truth[k]) for k in truth}
    print(case['name'], layout, routing, {k: f'{v:.1e}{"" if split[k] else " (no split kernel)"}' for k, v in err.items()})
    for k in truth:
        assert torch.isfinite(got[k]).all(), k
        if split[k]:
            assert 1e-5 < err[k] < 1e-2, (k, err[k])
        else:
            assert err[k] < 1e-4, (k, err[k])
    if routing == 'default' and case.get('groups', 1) == 1 and case['C'] % 64 == 0 and case['Co'] % 64 == 0 and \
            case['C'] >= 128 and case['Co'] >= 128:
        # the wide single-group layers run their contractions on the one-product kernels (the bias gradient is a plain sum)
        assert split['out'] and split['gx'] and split['gw'], split
    if split['out']:
        ref = _rounded_forward(x, w, b, off, mask, cfg).detach()
        d = (got['out'].double().cpu() - ref).abs() / ref.abs().max()
        e, frac = float(d.max()), float((d > 1e-4).double().mean())
        print(case['name'], layout, routing, f'forward vs rounded-column fp64 {e:.1e}, share beyond 1e-4 {frac:.1e}')
        assert frac < ROUNDED_FWD_FRAC and e < 1e-3, (e, frac)


# ---------------------------------------------------------------------------------- switching, reproducibility, training
def test_bf16_interlude_leaves_bf16x6_unchanged(math_mode):
    """'bf16x6' outputs and gradients of a deformable and a dense layer, bit-identical before and after a 'bf16' run that
    prepares (one-plane) images of the SAME weight tensors: the image caches are keyed on the mode."""
    from lsnet_amd import ops
    from lsnet_amd.ops.conv import conv2d
    dev = _dev()
    case = next(c for c in DCN_CASES if c['name'] == 'v2_head_p6')
    x, w, b, off, mask, go, cfg = _make(case, dev, seed=11)
    wp = torch.nn.Parameter(_cl(w.to(dev)))               # a parameter: the DCN image comes from the per-step cache
    torch.manual_seed(2)
    xc = _cl(torch.randn(2, 256, 25, 42, device=dev)).requires_grad_()
    wc = torch.nn.Parameter(_cl(torch.randn(256, 256, 3, 3, device=dev) / 48.))

    def run():
        xd, od, md = _cl(x.to(dev)).requires_grad_(), _cl(off.to(dev)), _cl(mask.to(dev))
        out = ops.dcn_multi([xd], [od], [md], wp, b.to(dev), cfg['stride'], cfg['pad'], cfg['dil'], cfg['groups'], cfg['dg'],
                            scales=[(1.0, 1.0)], pyramid=False)[0]
        res = [out.detach()] + [t.detach() for t in torch.autograd.grad(out, [xd, wp], _cl(go.to(dev)))]
        y = conv2d(xc, wc, None, 1, 1, 1)
        res += [y.detach()] + [t.detach() for t in torch.autograd.grad(y, [xc, wc], torch.ones_like(y))]
        torch.cuda.synchronize()
        return res
    math_mode('bf16x6')
    before = run()
    math_mode('bf16')
    mid = run()
    math_mode('bf16x6')
    after = run()
    for i, (p, q, m) in enumerate(zip(before, after, mid)):
        assert torch.equal(p, q), i
        assert not torch.equal(p, m), i   # the interlude did run in the other arithmetic


def test_bf16_training_step_is_bit_reproducible(math_mode):
    from lsnet_amd.data import synthetic_batch
    from lsnet_amd.model_zoo import build_lsnet
    dev = _dev()
    math_mode('bf16')

    def run():
        torch.manual_seed(3)
        model, _ = build_lsnet('bbox', 'r50')
        model = model.to(dev).to(memory_format=torch.channels_last).train()
        data = synthetic_batch('bbox', 2, 384, 480, boxes_per_img=5, num_classes=80, seed=11, device='cuda:0', channels_last=True)
        losses = model(**data)
        loss = sum(v if torch.is_tensor(v) else sum(v) for k, v in losses.items() if 'loss' in k)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    l1, g1 = run()
    l2, g2 = run()
    assert torch.isfinite(l1)
    assert torch.equal(l1, l2), (float(l1), float(l2))
    assert len(g1) > 100
    diff = [n for n in g1 if not torch.equal(g1[n], g2[n])]
    assert not diff, f'{len(diff)} of {len(g1)} parameter gradients differ between two identical steps, e.g. {diff[:4]}'


# 3x the worst relative deviation per term over the twenty iterations measured on the MI355X: total 0.13, classification
# 0.032, init 0.15, refine 0.27 (bf16 products move the trajectory early -- iteration 1 already 3e-2 -- and SGD carries it on)
CURVE_TOL = dict(loss=0.39, loss_cls=0.096, loss_bbox_init=0.45, loss_bbox_refine=0.81)


def test_bf16_training_curve_of_the_benchmark_model(math_mode):
    """The benchmark model's twenty-iteration curve (fixture train_curve_init0, the reference's run in fp32) in 'bf16':
    every iteration finite and within CURVE_TOL (3x the measured worst per term).  The weights after the run are not held
    to the fp32 fixture (rtol_weight 10): twenty steps of a different arithmetic are a different trajectory."""
    import numpy as np
    import tests.golden_cases as gc
    math_mode('bf16')
    worst = gc.train_curve_case(_dev(), early_tol=CURVE_TOL, late_tol=CURVE_TOL, rtol_weight=10.0, channels_last=True,
                                fixture='train_curve_init0', init0=True)
    assert np.isfinite(worst)
    print(f'bf16 benchmark-model curve: worst relative loss deviation over twenty iterations {worst:.2e}')
