"""Every backbone block variant as one stage on the MI355X against float64 autograd over the plain restatement of
tests/backbone_stage_cases.py: DCNv2 / DCNv1 in conv2, ResNeXt grouped conv2 (gconv.hip), grouped DCN, Res2Net Bottle2neck
(channel-slice inputs, running sums, the 3x3 pool of the last scale, the average-pool shortcut), style='caffe', dilation,
BasicBlock and GroupNorm norms -- output, input gradient and EVERY parameter gradient, each element under
bound(kind, e_host) = max(1e-5 output / 2e-5 gradient, 16 x e_host), in the math modes 'bf16x6' and 'fp32'.  conv_offset is
random, so the offsets differ per pixel and samples leave the map; the two conditions of the cases module (kink and lattice
clearance) are what lets the bound be a maximum over all elements with no outlier budget.

Further arms on a few cases: input without requires_grad, with_cp=True, the frozen stage (forward only), an NCHW-contiguous
input.  `test_routes` reads the library's launch log and counts the pooling calls, so that a case named for a kernel family is
known to have run it, and states which norms the fused BatchNorm kernel's own predicate declines (finding below).

Finding: `ops/batch_norm.py::_hip_ok` declines the Res2Net widths of this stage -- 52 channels (bns.*) and 208 (bn1): 256 is no
multiple of C / 4 -- so those eval-mode BatchNorms (+ ReLU) run as ATen's operators on the device, without the fall-back warning
the convolutions and pools give.  The cases stay and test_routes asserts the decline explicitly; the numbers below include it.

MEASURED (MI355X; device error against float64 / e_host = the fp32 host evaluation's own error / their ratio; per case and mode
the output, the input gradient and the worst parameter gradient by share of its bound; every tensor of every case and mode is in
profiles/backbone_stage_errors.txt):
  case           mode   output                    input gradient            worst parameter gradient
  r_v2_s2        bf16x6 6.6e-07 / 7.5e-07 / 0.9   9.4e-07 / 1.2e-06 / 0.8   2.2e-06 / 1.2e-06 / 1.8  0.conv2.conv_offset.bias (0.11 of its bound)
  r_v2_s2        fp32   6.6e-07 / 7.5e-07 / 0.9   9.1e-07 / 1.2e-06 / 0.8   2.2e-06 / 1.2e-06 / 1.8  0.conv2.conv_offset.bias (0.11 of its bound)
  r_v2_dg4_caffe bf16x6 5.2e-07 / 4.7e-07 / 1.1   1.1e-06 / 8.7e-07 / 1.2   2.2e-06 / 1.3e-06 / 1.7  1.bn1.weight (0.11 of its bound)
  r_v2_dg4_caffe fp32   5.2e-07 / 4.7e-07 / 1.1   1.1e-06 / 8.7e-07 / 1.3   2.9e-06 / 1.3e-06 / 2.2  1.bn1.weight (0.14 of its bound)
  r_v1_dil2      bf16x6 6.6e-07 / 6.0e-07 / 1.1   1.1e-06 / 1.1e-06 / 1.0   1.9e-06 / 1.1e-06 / 1.8  0.conv3.weight (0.10 of its bound)
  r_v1_dil2      fp32   6.6e-07 / 6.0e-07 / 1.1   1.0e-06 / 1.1e-06 / 0.9   1.9e-06 / 1.1e-06 / 1.8  0.conv3.weight (0.10 of its bound)
  x_c4_s2        bf16x6 4.8e-07 / 4.6e-07 / 1.1   3.3e-07 / 3.5e-07 / 0.9   7.0e-07 / 4.5e-07 / 1.5  0.conv2.weight (0.04 of its bound)
  x_c4_s2        fp32   4.8e-07 / 4.6e-07 / 1.1   3.3e-07 / 3.5e-07 / 0.9   7.1e-07 / 4.5e-07 / 1.6  0.conv2.weight (0.04 of its bound)
  x_c32_s1       bf16x6 5.2e-07 / 3.1e-07 / 1.7   4.0e-07 / 3.1e-07 / 1.3   7.7e-07 / 1.9e-07 / 3.9  0.bn1.weight (0.04 of its bound)
  x_c32_s1       fp32   5.2e-07 / 3.1e-07 / 1.7   4.0e-07 / 3.1e-07 / 1.3   7.7e-07 / 1.9e-07 / 3.9  0.bn1.weight (0.04 of its bound)
  x_dcn_c8_s2    bf16x6 8.2e-07 / 8.5e-07 / 1.0   1.9e-06 / 1.3e-06 / 1.4   2.7e-06 / 9.6e-07 / 2.8  2.bn1.weight (0.13 of its bound)
  x_dcn_c8_s2    fp32   8.2e-07 / 8.5e-07 / 1.0   1.9e-06 / 1.3e-06 / 1.4   2.7e-06 / 9.6e-07 / 2.8  2.bn1.weight (0.13 of its bound)
  x_dcn_c16_s1   bf16x6 9.8e-07 / 6.9e-07 / 1.4   2.3e-06 / 1.9e-06 / 1.2   3.1e-06 / 1.5e-06 / 2.0  1.bn1.bias (0.13 of its bound)
  x_dcn_c16_s1   fp32   9.8e-07 / 6.9e-07 / 1.4   2.3e-06 / 1.9e-06 / 1.2   3.1e-06 / 1.5e-06 / 2.0  1.bn1.bias (0.13 of its bound)
  r2_s2          bf16x6 5.2e-07 / 3.7e-07 / 1.4   6.8e-07 / 6.0e-07 / 1.1   2.1e-06 / 3.9e-07 / 5.3  1.bn1.bias (0.10 of its bound)
  r2_s2          fp32   5.2e-07 / 3.7e-07 / 1.4   6.8e-07 / 6.0e-07 / 1.1   2.1e-06 / 3.9e-07 / 5.3  1.bn1.bias (0.10 of its bound)
  r2_dcn_s2      bf16x6 7.0e-07 / 6.5e-07 / 1.1   1.4e-06 / 1.5e-06 / 1.0   2.9e-06 / 1.3e-06 / 2.3  0.conv3.weight (0.14 of its bound)
  r2_dcn_s2      fp32   7.0e-07 / 6.5e-07 / 1.1   1.5e-06 / 1.5e-06 / 1.0   2.7e-06 / 1.3e-06 / 2.1  0.conv3.weight (0.13 of its bound)
  r2_dcn_s1      bf16x6 1.1e-06 / 9.3e-07 / 1.2   4.0e-06 / 2.9e-06 / 1.4   5.0e-06 / 1.6e-06 / 3.1  1.convs.0.weight (0.20 of its bound)
  r2_dcn_s1      fp32   1.1e-06 / 9.3e-07 / 1.2   4.1e-06 / 2.9e-06 / 1.4   5.1e-06 / 1.6e-06 / 3.2  1.convs.0.weight (0.20 of its bound)
  basic_s2       bf16x6 4.7e-07 / 3.1e-07 / 1.5   4.4e-07 / 5.1e-07 / 0.9   5.3e-07 / 2.6e-07 / 2.0  0.bn1.bias (0.03 of its bound)
  basic_s2       fp32   4.7e-07 / 3.1e-07 / 1.5   4.4e-07 / 5.1e-07 / 0.9   5.3e-07 / 2.6e-07 / 2.0  0.bn1.bias (0.03 of its bound)
  gn_s2          bf16x6 4.5e-07 / 3.4e-07 / 1.3   3.7e-07 / 4.8e-07 / 0.8   5.7e-07 / 5.0e-07 / 1.1  0.gn1.weight (0.03 of its bound)
  gn_s2          fp32   4.5e-07 / 3.4e-07 / 1.3   3.7e-07 / 4.8e-07 / 0.8   5.7e-07 / 5.0e-07 / 1.1  0.gn1.weight (0.03 of its bound)
  further arms (bf16x6), the worst tensor by share of its bound:
  r_v2_s2        no-input-grad  2.2e-06 / 1.2e-06 / 1.8  0.conv2.conv_offset.bias (0.11 of its bound)
  x_c4_s2        no-input-grad  4.8e-07 / 4.6e-07 / 1.1  out (0.05 of its bound)
  r2_dcn_s2      no-input-grad  2.8e-06 / 1.3e-06 / 2.1  0.conv3.weight (0.13 of its bound)
  r_v2_s2        with_cp        2.2e-06 / 1.2e-06 / 1.8  0.conv2.conv_offset.bias (0.11 of its bound)
  r2_dcn_s2      with_cp        3.0e-06 / 1.3e-06 / 2.3  0.conv3.weight (0.15 of its bound)
  r_v2_s2        frozen         5.2e-07 / 7.5e-07 / 0.7  out (0.04 of its bound)
  x_c32_s1       frozen         5.1e-07 / 3.1e-07 / 1.7  out (0.05 of its bound)
  r2_s2          frozen         6.2e-07 / 3.7e-07 / 1.7  out (0.06 of its bound)
  r_v2_s2        nchw           2.2e-06 / 1.2e-06 / 1.8  0.conv2.conv_offset.bias (0.11 of its bound)
  x_c4_s2        nchw           4.8e-07 / 4.6e-07 / 1.1  out (0.05 of its bound)
  r2_s2          nchw           2.1e-06 / 3.9e-07 / 5.3  1.bn1.bias (0.10 of its bound)
  over all 1180 comparisons: largest share of a bound 0.20, largest ratio to e_host 5.3, largest e_host 4.6e-06
"""
import contextlib
import copy

import pytest
import torch

from tests import backbone_stage_cases as C

pytestmark = pytest.mark.gpu
CL = torch.channels_last
MODES = ['bf16x6', 'fp32']
R2_CASES = [n for n in C.CASES if n.startswith('r2_')]


@contextlib.contextmanager
def _math(mode):
    from lsnet_amd import _lib
    old = _lib.get_math_mode()
    try:
        _lib.set_math_mode(mode)
        yield
    finally:
        _lib.set_math_mode(old)


def _device_stage(ref, with_cp=False):
    layer = C.as_trained(copy.deepcopy(ref.layer)).to('cuda:0').to(memory_format=CL)
    for blk in layer:
        blk.with_cp = with_cp
    return layer


def _run(ref, layer, x):
    """forward, backward under the case's upstream gradient -> {'out', 'x' (if x asks for it), parameter name: gradient}"""
    y = layer(x)
    y.backward(ref.go.to(y.device))
    torch.cuda.synchronize()
    got = {'out': y.detach()}
    if x.requires_grad:
        got['x'] = x.grad
    for k, p in layer.named_parameters():
        assert p.grad is not None, k
        got[k] = p.grad
    return got


def _check(tag, ref, got):
    rows = C.compare(ref, got)
    C.report(tag, rows)
    assert not C.failures(rows), (tag, C.failures(rows))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(C.CASES))
def test_stage_equals_fp64_autograd(name, mode):
    from lsnet_amd.models.backbones import resnet as R
    ref = C.reference(name)
    layer = _device_stage(ref)
    x = ref.x.to('cuda:0').contiguous(memory_format=CL).requires_grad_()
    assert not any(R.fused_block_ok(b, x) for b in layer)     # (the dense fused node has its own test: tests/test_resblock_gpu.py)
    with _math(mode):
        got = _run(ref, layer, x)
    assert set(got) == set(ref.f64)
    _check(f'{name} {mode}', ref, got)


@pytest.mark.parametrize('name', ['r_v2_s2', 'x_c4_s2', 'r2_dcn_s2'])
def test_input_without_grad(name):
    """the first trainable stage behind a frozen one: no data gradient leaves the stage, every parameter gradient holds"""
    ref = C.reference(name)
    layer = _device_stage(ref)
    with _math('bf16x6'):
        got = _run(ref, layer, ref.x.to('cuda:0').contiguous(memory_format=CL))
    assert set(got) == set(ref.f64) - {'x'}
    _check(f'{name} no-input-grad', ref, got)


@pytest.mark.parametrize('name', ['r_v2_s2', 'r2_dcn_s2'])
def test_with_checkpointing(name):
    ref = C.reference(name)
    layer = _device_stage(ref, with_cp=True)
    with _math('bf16x6'):
        got = _run(ref, layer, ref.x.to('cuda:0').contiguous(memory_format=CL).requires_grad_())
    _check(f'{name} with_cp', ref, got)


@pytest.mark.parametrize('name', ['r_v2_s2', 'x_c32_s1', 'r2_s2'])
def test_frozen_stage_forward(name):
    """eval() with frozen parameters: the dense conv + BatchNorm pairs take conv_bn_act_frozen; forward only"""
    ref = C.reference(name)
    layer = _device_stage(ref).eval()
    for p in layer.parameters():
        p.requires_grad_(False)
    with _math('bf16x6'):
        y = layer(ref.x.to('cuda:0').contiguous(memory_format=CL))
        torch.cuda.synchronize()
    assert not y.requires_grad
    _check(f'{name} frozen', ref, {'out': y})


@pytest.mark.parametrize('name', ['r_v2_s2', 'x_c4_s2', 'r2_s2'])
def test_nchw_input(name):
    ref = C.reference(name)
    layer = _device_stage(ref)
    x = ref.x.to('cuda:0').contiguous().requires_grad_()
    assert not x.is_contiguous(memory_format=CL)
    with _math('bf16x6'):
        got = _run(ref, layer, x)
    _check(f'{name} nchw', ref, got)


POOL_CALLS = {'r2_s2': 2, 'r2_dcn_s2': 2, 'r2_dcn_s1': 1}      # the last scale's 3x3 pool (stride 2 only) + the shortcut's pool


@pytest.mark.parametrize('name', list(C.CASES))
def test_routes(name, monkeypatch):
    """The trainable arm runs the kernel families the case is named for, and nothing leaves for ATen with a warning."""
    from lsnet_amd import _lib
    from lsnet_amd.ops import batch_norm
    from lsnet_amd.ops import conv as conv_ops
    from lsnet_amd.ops.backend import get_backend
    ref = C.reference(name)
    layer = _device_stage(ref)
    x = ref.x.to('cuda:0').contiguous(memory_format=CL).requires_grad_()
    be = get_backend(x)
    calls, fallbacks = {}, []
    for fn in ('avg_pool2d_forward', 'avg_pool2d_backward'):
        def wrapper(*a, _f=getattr(be, fn), _n=fn, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(be, fn, wrapper, raising=False)
    monkeypatch.setattr(conv_ops, '_warn_aten_fallback', lambda what, t, detail: fallbacks.append((what, detail)))
    with _math('bf16x6'):
        try:
            _lib.prof_enable(1)
            _run(ref, layer, x)
            log = _lib.prof_read()
        finally:
            _lib.prof_enable(0)
    n = {f: log.get(f, {}).get('launches', 0) for f in _lib.PROF_FAMILIES}
    print(f'STAGE {name} routes {n} pools {calls}')
    assert not fallbacks, fallbacks
    dcn = ('dcn_fwd', 'dcn_bwd_data', 'dcn_wgrad')
    if name in C.DCN_CASES:
        assert all(n[f] > 0 for f in dcn) and n['gconv'] == 0, n
    else:
        assert not any(n[f] for f in dcn), n
    if name.startswith('x_c'):
        assert n['gconv'] >= 3 * len(layer), n          # forward, data and weight gradient of every block's conv2
    elif not name.startswith('x_dcn'):
        assert n['gconv'] == 0, n
    if name == 'gn_s2':
        assert n['norm'] > 0, n
    want = POOL_CALLS.get(name, 0)
    assert calls == ({'avg_pool2d_forward': want, 'avg_pool2d_backward': want} if want else {}), calls
    # which eval-mode BatchNorms the fused norm kernel's own predicate declines (they run ATen's batch_norm + relu on the device)
    declined = {k for k, m in layer.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and not batch_norm._hip_ok(
        m, torch.empty(1, m.num_features, 1, 1, device='cuda:0').contiguous(memory_format=CL), None)}
    if name in R2_CASES:
        assert declined == {f'{i}.{k}' for i in range(len(layer)) for k in ('bn1', 'bns.0', 'bns.1', 'bns.2')}, declined
    else:
        assert not declined, declined
