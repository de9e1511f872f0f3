"""Every backward pass of lsnet_amd/ops under partial requests and onto non-zero gradient sinks, against the fp64 references of
tests/backward_request_cases.py (the deformable family: the CPU oracle).

A. Which gradients are asked for: `requires_grad` flags on the leaves and `.backward()`, as frozen parameters and detached
   inputs do in training.  What is asked for equals the reference at the tolerance the operator's own test uses; every other
   leaf's .grad stays None.  For the deformable family the request picks the kernels (csrc/dcn_route.h route_backward): offsets
   without their input leave the atomic-free gather for the scatter kernels with a NULL grad_input, no data gradient at all
   leaves the weight gradient without the gather pass's tap table.
B. Where parameter gradients go: views of one arena registered as gradient sinks (ops/grad_sink.py), prefilled with non-zero
   values between canary floats.  The `accumulate = 1` form of every entry point must ADD; a route that overwrote, added twice,
   wrote a frozen parameter's view or a neighbour's would pass every test that zeroes its buffers first.
C. One weight with two contributions in one graph, plainly and with deferred reduces (lsn_wgrad_defer: the second call finds a
   queued reduce for its gradient): base + g1 + g2 both times, and the same bits.

Each test prints one `REQ ...` line per (operator, case, mode) with the worst error per gradient (pytest -s)."""
import collections
import contextlib
import ctypes

import pytest
import torch

from tests import backward_request_cases as br
from tests.test_ops_gpu import KERNEL_CHOICES, TOL as DCN_TOL

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
LSN_ERR_UNSUPPORTED = -2


def _dev():
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'
    return torch.device('cuda:0')


@contextlib.contextmanager
def _math(mode, debug_word=0):
    from lsnet_amd import _lib
    old = _lib.get_math_mode()
    try:
        _lib.set_debug_word(debug_word)
        _lib.set_math_mode(mode)
        yield
    finally:
        _lib.set_math_mode(old)
        _lib.set_debug_word(0)


def _put(v, nhwc=True):
    v = v.detach().float().to(_dev(), copy=True)        # (a tensor of its own: the shared reference is never a leaf)
    return v.contiguous(memory_format=_CL) if (nhwc and v.dim() == 4) else v.contiguous()


def _tensors(case, ref, req, nhwc=True):
    """leaves (parameters as nn.Parameter, requires_grad as `req` says) and constants of the case on the device"""
    params = br.param_names(case)
    leaves = collections.OrderedDict()
    for n, v in ref.leaves.items():
        v = _put(v, nhwc)
        leaves[n] = torch.nn.Parameter(v, requires_grad=n in req) if n in params else v.requires_grad_(n in req)
    t = {n: _put(v) for n, v in ref.consts.items()}
    t.update(leaves)
    return leaves, t


def _bn(t, C):
    bn = torch.nn.BatchNorm2d(C, eps=br.BN_EPS).to(_dev()).eval()
    bn.weight, bn.bias = t['gamma'], t['beta']
    with torch.no_grad():
        bn.running_mean.copy_(t['mean'])
        bn.running_var.copy_(t['var'])
    return bn


def _cat_px(ts):
    """per-level (B, C, H, W) -> (B, C, N_all, 1), the pixel rows of all levels back to back (LSHead._cat_px)"""
    B, C = ts[0].shape[:2]
    return torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, C) for m in ts], dim=1).unsqueeze(2).permute(0, 3, 1, 2)


def _outputs(case, t):
    """the operator of the case through lsnet_amd.ops on the device tensors `t` -> one tensor per output of the reference"""
    from lsnet_amd import ops
    from lsnet_amd.ops import conv as C
    from lsnet_amd.ops.batch_norm import bn_act, _hip_ok as bn_hip_ok
    from lsnet_amd.ops.group_norm import GroupNorm, _hip_ok as gn_hip_ok
    c = br.cfg_of(case)
    if case.op == 'conv2d':
        return [C.conv2d(t['x'], t['w'], t.get('b'), c['s'], c['p'], 1, relu=c['relu'])]
    if case.op == 'conv2d_multi':
        n = len(c['sizes'])
        return C.conv2d_multi([t[f'x{i}'] for i in range(n)], t['w'], t['b'], c['p'], 1, c['relu'],
                              [t[f'r{i}'] for i in range(n)] if c['res'] else None)
    if case.op == 'gconv':
        assert C.hip_group_conv_ok(t['x'], t['w'], (c['s'],) * 2, (c['p'],) * 2, (1, 1), c['G'])
        return [C._GroupConvFn.apply(t['x'], t['w'], t.get('b'), c['s'], c['p'], 1, c['G'])]
    if case.op in ('conv_bn_act', 'conv_bn_pair'):
        conv = C.Conv2d(c['C'], c['Co'], c['k'], stride=c['s'], padding=c['p'], bias=False).to(_dev())
        conv.weight = t['w']
        bn = _bn(t, c['Co'])
        if case.op == 'conv_bn_pair':      # two calls: the three parameters are used twice in one graph
            ys = [C.conv_bn_act(conv, bn, t[f'x{i}'], relu=c['relu']) for i in range(len(c['sizes']))]
        else:
            ys = [C.conv_bn_act(conv, bn, t['x'], relu=c['relu'], residual=t.get('residual'))]
        assert all(y is not None for y in ys), 'conv_bn_act declined the pair'
        return ys
    if case.op == 'bn_act':
        bn = _bn(t, c['C'])
        assert bn_hip_ok(bn, t['x'], t.get('residual'))
        return [bn_act(bn, t['x'], relu=c['relu'], residual=t.get('residual'))]
    if case.op == 'gn':
        m = GroupNorm(c['G'], c['C'], eps=br.GN_EPS).to(_dev())
        m.weight, m.bias = t['gamma'], t['beta']
        xs = [t[f'x{i}'] for i in range(len(c['sizes']))]
        assert all(gn_hip_ok(x, c['C'], c['G']) for x in xs)
        return [m.forward_cat_px(xs, relu=c['relu'])] if c['cat'] else m.forward_multi(xs, relu=c['relu'])
    if case.op == 'pack':
        pack = ops.ModulatedDeformConvPack(c['C'], c['Co'], 3, 1, 1).to(_dev())
        pack.weight, pack.bias, pack.conv_offset.weight, pack.conv_offset.bias = t['weight'], t['bias'], t['w_off'], t['b_off']
        return pack.forward_multi([t[f'x{i}'] for i in range(len(c['sizes']))])
    return br.dcn_outputs(case, t)


def _upstream(case, ref, nhwc=True):
    gos = [None if g is None else _put(g, nhwc) for g in ref.gos]
    if case.op == 'gn' and br.cfg_of(case)['cat']:
        return [_cat_px(gos)]
    return gos


def _reference_outputs(case, ref):
    return [_cat_px(ref.ys)] if (case.op == 'gn' and br.cfg_of(case)['cat']) else ref.ys


def _line(what, worst):
    print(f'REQ {what} ' + ' '.join(f'{n} {e:.2e}' for n, e in worst.items()))


def _sweep(what, case, reqs, tol, fwd_tol, unused=(), nhwc=True):
    """every request of `reqs` on the case: forward output, requested gradients, None for the rest; prints the worst errors"""
    ref = br.reference(case, unused)
    worst = collections.OrderedDict()
    for req in reqs:
        leaves, t = _tensors(case, ref, req, nhwc)
        outs = _outputs(case, t)
        for o, r in zip(outs, _reference_outputs(case, ref)):
            assert tuple(o.shape) == tuple(r.shape)
            worst['y'] = max(worst.get('y', 0.0), br.rel_diff(o.detach().double().cpu(), r))
            assert worst['y'] < fwd_tol, (what, req, worst['y'])
        got = br.backward(outs, _upstream(case, ref, nhwc), leaves)
        torch.cuda.synchronize()
        for n, e in br.check_request(got, ref.grads, req, tol).items():
            worst[n] = max(worst.get(n, 0.0), e)
    _line(f'{what} {case.op} {case.name} ({len(reqs)} requests)', worst)
    return worst


# ================================================================================== A. partial requests
@pytest.fixture(params=['bf16x6', 'bf16x3'])
def split_mode(request):
    with _math(request.param):
        yield request.param


def _conv_tol(mode):       # tests/test_conv_geometry_gpu.py _tol
    return 3e-6 if mode == 'bf16x6' else 5e-5


@pytest.mark.parametrize('case', br.CONV2D, ids=[c.name for c in br.CONV2D])
def test_conv2d_requests(case, split_mode):
    """_ConvFn: every non-empty subset of (x, w, b): the data gradient alone (with its zero-filter padding for Co = 27), the
    weight without the bias and the bias without the weight out of the one weight-gradient launch."""
    _sweep(split_mode, case, br.requests(br.leaf_names(case)), _conv_tol(split_mode), _conv_tol(split_mode))


@pytest.mark.parametrize('case', br.CONV_MULTI, ids=[c.name for c in br.CONV_MULTI])
def test_conv2d_multi_requests(case, split_mode):
    """_ConvMultiFn: need_x patterns TFT / FFF / TTT, w only, b only, one residual only, all; then one output left out of the
    loss (its upstream gradient is materialised as zeros)."""
    tol = _conv_tol(split_mode)
    _sweep(split_mode, case, br.conv_multi_requests(case), tol, tol)
    _sweep(split_mode + ' output 1 unused', case, [br.leaf_names(case), ('x0', 'x1', 'w')], tol, tol, unused=(1,))


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
@pytest.mark.parametrize('case', br.GCONV, ids=[c.name for c in br.GCONV])
def test_grouped_conv_requests(case, mode):
    """_GroupConvFn (exact fp32 in every math mode): 1e-6 forward, 2e-6 gradients as test_grouped_conv2d_matches_torch."""
    with _math(mode):
        _sweep(mode, case, br.requests(br.leaf_names(case)), 2e-6, 1e-6)


@pytest.mark.parametrize('case', br.CONV_BN, ids=[c.name for c in br.CONV_BN])
def test_conv_bn_act_requests(case, split_mode):
    """_ConvBnActFn: wgrad_bn's `need` triple and the data / residual gradients, gamma with a 0 and a 1e-6 channel; 5e-6 / 5e-4
    as test_conv_bn_act_folded_geometry."""
    tol = 5e-6 if split_mode == 'bf16x6' else 5e-4
    leaves = br.leaf_names(case)
    reqs = br.requests(leaves) + [('gamma', 'beta'), ('w', 'gamma', 'beta'), ('x', 'w')]
    _sweep(split_mode, case, [r for i, r in enumerate(reqs) if r not in reqs[:i]], tol, tol)


@pytest.mark.parametrize('case', br.BN, ids=[c.name for c in br.BN])
def test_bn_act_requests(case):
    """_BnActFn / lsn_bn_eval_act_backward with any of grad_x, grad_residual, grad_gamma + grad_beta NULL; gamma without beta
    and beta without gamma come out of the one parameter pass.  1e-6 forward, 2e-5 gradients as test_bn_eval_act_matches_torch."""
    leaves = br.leaf_names(case)
    reqs = br.requests(leaves) + [('gamma', 'beta'), ('x', 'gamma'), ('x', 'beta')]
    _sweep('-', case, [r for i, r in enumerate(reqs) if r not in reqs[:i]], 2e-5, 1e-6)


@pytest.mark.parametrize('case', br.GN, ids=[c.name for c in br.GN])
def test_group_norm_requests(case):
    """GroupNorm.forward_multi / forward_cat_px: x0 only, x1 only, gamma only, beta only, the parameters only, the inputs only,
    all; forward_multi also with one level's output unused.  1e-5 / 2e-5 / ptol as test_group_norm_matches_torch."""
    c = br.cfg_of(case)
    ptol = 2e-5 if (c['C'] // c['G']) % 4 == 0 else 6e-5
    tol = {None: 2e-5, 'gamma': ptol, 'beta': ptol}
    _sweep('-', case, br.GN_REQUESTS, tol, 1e-5)
    if not c['cat']:
        _sweep('- output 1 unused', case, [br.leaf_names(case), ('x0', 'gamma')], tol, 1e-5, unused=(1,))


# ---------------------------------------------------------------------------------- the deformable family
def _dcn_abi(case, want, grad_weight=False, grad_bias=False):
    """One channels-last level of a 'dcn' case at the C ABI, built as HipBackend builds it: shape, levels and everything that
    must stay alive.  want: the data gradients that get a buffer; the others are NULL."""
    from lsnet_amd import _lib
    from lsnet_amd.ops.hip_backend import HipBackend, _strides
    ref = br.reference(case)
    c = br.cfg_of(case)
    d = {n: _put(v) for n, v in ref.leaves.items()}
    d['go'] = _put(ref.gos[0])
    x, off, mask, w = d['x'], d['off'], d.get('mask'), d['w']
    lib = _lib.load()
    shape = HipBackend._shape(w, dict(stride=1, pad=1, dil=1, groups=c['groups'], dg=1))
    levels = (_lib.DcnLevel * 1)()
    L = levels[0]
    L.input, L.offset, L.mask, L.grad_output = x.data_ptr(), off.data_ptr(), _lib.ptr(mask), d['go'].data_ptr()
    L.off_st = _strides(off)
    if mask is not None:
        L.mask_st = _strides(mask)
    L.B, L.H, L.W, L.Ho, L.Wo = x.shape[0], x.shape[2], x.shape[3], x.shape[2], x.shape[3]
    L.scale_h = L.scale_w = 1.0
    d['gx'] = torch.full_like(x, float('nan')) if 'x' in want else None
    d['goff'] = torch.full_like(off, float('nan')) if 'off' in want else None
    d['gmask'] = torch.full_like(mask, float('nan')) if ('mask' in want and mask is not None) else None
    L.grad_input, L.grad_offset, L.grad_mask = _lib.ptr(d['gx']), _lib.ptr(d['goff']), _lib.ptr(d['gmask'])
    d['gw'] = torch.full_like(w, float('nan')) if grad_weight else None
    d['gb'] = torch.full((w.shape[0],), float('nan'), device=w.device) if grad_bias else None
    if _lib.split_math() and c['groups'] == 1:
        d['ws'] = torch.empty(2 * w.numel(), device=w.device)
        shape.workspace = d['ws'].data_ptr()
    nbytes = int(lib.lsn_dcn_backward_workspace_bytes(ctypes.byref(shape), 1, levels))
    if nbytes > 0:
        d['gws'] = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
        shape.gather_workspace, shape.gather_workspace_bytes = d['gws'].data_ptr(), nbytes
    return lib, shape, levels, d, nbytes, ref


def test_dcn_cases_sit_on_the_routes_they_are_named_for():
    """'mm' and 'mm_wg' with every gradient requested in 'bf16x6': lsn_dcn_prepared_ok(backward) == 1, so the cases cannot leave
    the matrix-pipe data gradient unnoticed; lsn_dcn_pitched_ok(backward) -- GATHER_MM and WG_MM -- is 1 for 'mm_wg' alone.
    'xn' (Co % 128), 'grouped' and 'v1' answer 0 to the weight-gradient question: the split and the grouped kernels."""
    with _math('bf16x6'):
        got = {}
        for name, case in br.DCN.items():
            lib, shape, levels, d, nbytes, _ = _dcn_abi(case, ('x', 'off', 'mask'), True, br.cfg_of(case)['bias'])
            got[name] = (nbytes > 0, lib.lsn_dcn_prepared_ok(ctypes.byref(shape), 1, levels, 1),
                         lib.lsn_dcn_pitched_ok(ctypes.byref(shape), 1, levels, 1))
        print('REQ dcn routes (gather workspace, prepared_ok, pitched_ok):', got)
        assert got['mm'][:2] == (True, 1) and got['mm_wg'] == (True, 1, 1), got
        assert got['mm'][2] == 0 and got['xn'][2] == 0 and got['grouped'][1:] == (0, 0) and got['v1'][2] == 0, got


DCN_CHOICES = ['default', 'x3_atomic_fallbacks', 'math_fp32']


@pytest.mark.parametrize('choice', DCN_CHOICES)
@pytest.mark.parametrize('name', list(br.DCN))
def test_dcn_multi_requests(name, choice):
    """_DCNFunction on one level: under the defaults all 31 subsets for 'xn' (channels-last, and the route requests in NCHW),
    DCN_ROUTE_REQUESTS + all for the rest; the route requests + all under the atomic fallbacks and in exact fp32.  1e-4 against
    the oracle as test_dcn_forward_backward."""
    case = br.DCN[name]
    mode, word = KERNEL_CHOICES[choice]
    with _math(mode, word):
        _sweep(f'{choice} nhwc', case, br.dcn_requests(case, everything=(name == 'xn' and choice == 'default')), DCN_TOL, DCN_TOL)
        if name == 'xn':
            _sweep(f'{choice} nchw', case, br.dcn_requests(case), DCN_TOL, DCN_TOL, nhwc=False)


@pytest.mark.parametrize('choice', DCN_CHOICES)
def test_dcn_pyramid_requests(choice):
    """One PyramidDeformConv-style call of three levels, source A under two of them: A with B detached and the reverse, the
    offsets of all levels or of level 0 alone (levels with and without grad_input / grad_offset in ONE call: gather_plan skips
    the former, route_backward sends the call to the scatter kernels for the latter), weight on and off; then with level 1's
    output unused."""
    mode, word = KERNEL_CHOICES[choice]
    with _math(mode, word):
        _sweep(choice, br.DCN_PYR, br.PYR_REQUESTS, DCN_TOL, DCN_TOL)
        _sweep(choice + ' output 1 unused', br.DCN_PYR, [br.PYR_REQUESTS[-1], ('xA', 'w')], DCN_TOL, DCN_TOL, unused=(1,))


def test_dcn_pack_requests():
    """_DCNPackFn over two maps: x frozen with every parameter trainable, conv_offset's parameters alone, the main weight
    alone, x alone, all -- 1e-5 against the explicit fp64 composition (F.conv2d -> torch_dcn with the sigmoid)."""
    with _math('bf16x6'):
        _sweep('bf16x6', br.PACK, br.PACK_REQUESTS, 1e-5, 1e-5)


def test_dcn_request_decides_which_passes_are_launched():
    """The library's launch log: a request without any data gradient records no dcn_bwd_data launch, one without weight and
    bias no dcn_wgrad launch."""
    from lsnet_amd import _lib
    case = br.DCN['xn']
    ref = br.reference(case)
    launches = {}
    with _math('bf16x6'):
        try:
            for req in (('w', 'b'), ('x', 'off', 'mask'), br.DCN_LEAVES):
                leaves, t = _tensors(case, ref, req)
                outs = br.dcn_outputs(case, t)
                _lib.prof_enable(1)
                br.backward(outs, _upstream(case, ref), leaves)
                torch.cuda.synchronize()
                log = _lib.prof_read()
                launches[req] = {f: log.get(f, {}).get('launches', 0) for f in ('dcn_bwd_data', 'dcn_wgrad')}
        finally:
            _lib.prof_enable(0)
    print('REQ dcn launches', launches)
    assert launches[('w', 'b')]['dcn_bwd_data'] == 0 and launches[('w', 'b')]['dcn_wgrad'] > 0, launches
    assert launches[('x', 'off', 'mask')]['dcn_wgrad'] == 0 and launches[('x', 'off', 'mask')]['dcn_bwd_data'] > 0, launches
    assert all(v > 0 for v in launches[br.DCN_LEAVES].values()), launches


def test_dcn_c_entry_with_null_gradients():
    """lsn_dcn_backward on one level of 'xn' with grad_input = NULL and grad_offset set (both documented "may be NULL"):
    lsn_dcn_backward_workspace_bytes promises 0, the call returns 0 and writes the reference grad_offset and nothing else;
    grad_bias with grad_weight = NULL is refused before any launch."""
    from lsnet_amd import _lib
    case = br.DCN['xn']
    with _math('bf16x6'):
        lib, shape, levels, d, nbytes, ref = _dcn_abi(case, ('off',))
        assert nbytes == 0
        rc = lib.lsn_dcn_backward(ctypes.byref(shape), 1, levels, d['w'].data_ptr(), None, None, 1, _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.lsn_last_error()
        e = br.rel_diff(d['goff'].double().cpu(), ref.grads['off'])
        print(f'REQ dcn C entry grad_input NULL: goff {e:.2e}')
        assert e < DCN_TOL
        lib, shape, levels, d, nbytes, ref = _dcn_abi(case, ('off',), grad_weight=False, grad_bias=True)
        rc = lib.lsn_dcn_backward(ctypes.byref(shape), 1, levels, d['w'].data_ptr(), None, d['gb'].data_ptr(), 1, _lib.stream())
        torch.cuda.synchronize()
        assert rc == LSN_ERR_UNSUPPORTED and b'grad_bias without grad_weight is not supported' in lib.lsn_last_error()
        assert bool(torch.isnan(d['gb']).all()) and bool(torch.isnan(d['goff']).all())       # refused: nothing was launched


# ================================================================================== B. non-zero sinks
def _run_sunk(case, state, tol, unused=(), outputs=None, defer=False, uses=1):
    """state 'all_sunk': every trainable parameter has a sink (the accumulate = 1 call); 'weight_only': only the first one
    (the classic path + AccumulateGrad must end in the same buffer with the same value); 'one_frozen': the last parameter is
    frozen after registration (its view stays bit-identical).  defer: the backward pass runs between lsn_wgrad_defer(64) and
    lsn_wgrad_defer(0).  uses: calls of one graph that share the parameters.  Returns (errors, arena after)."""
    from lsnet_amd import _lib
    from lsnet_amd.ops import grad_sink
    ref = br.reference(case, unused)
    names = br.param_names(case)
    leaves, t = _tensors(case, ref, br.leaf_names(case))
    params = collections.OrderedDict((n, leaves[n]) for n in names)
    views, before, index = br.arena(params, ref.grads, seed=case.seed)
    sunk = names[:1] if state == 'weight_only' else names
    frozen = names[-1:] if state == 'one_frozen' else ()
    done, returned = collections.Counter(), collections.Counter()
    for n in sunk:
        grad_sink.register(params[n], views[n], on_done=lambda p, n=n: done.update([n]))
        params[n].grad = views[n]
    for n in frozen:
        params[n].requires_grad_(False)
    for n in names:
        if n not in frozen:
            # (a leaf's hook also runs for an undefined gradient, with None: only tensors count as returned)
            params[n].register_hook(lambda g, n=n: returned.update([n] if g is not None else []))
    outs = (outputs or _outputs)(case, t)
    try:
        if defer:
            _lib.wgrad_defer(64)
        br.backward(outs, _upstream(case, ref), {})
    finally:
        if defer:
            _lib.wgrad_defer(0)      # (flushes the queued reduces and ends the mode)
    torch.cuda.synchronize()
    for n in sunk:
        assert params[n].grad.data_ptr() == views[n].data_ptr(), n
    loose = tuple(n for n in names if n not in sunk)
    for n in loose:       # no sink: a gradient tensor of its own, the arena's view untouched
        assert br.rel_diff(params[n].grad.double().cpu(), ref.grads[n]) < br.tol_of(tol, n), n
    errs = br.check_sunk(index['flat'], before, ref.grads, tol, index, frozen=tuple(frozen) + loose)
    if state == 'all_sunk':      # the Function returned None for every sunk parameter and told the sinks' owner once per use
        assert not returned and all(done[n] == uses for n in names), (returned, done)
    return errs, index['flat']


SUNK_STATES = ['all_sunk', 'weight_only', 'one_frozen']
_GN_TOL = lambda case: {None: 2e-5 if (br.cfg_of(case)['C'] // br.cfg_of(case)['G']) % 4 == 0 else 6e-5}
SUNK_CASES = [(c, 3e-6) for c in br.CONV2D + br.CONV_MULTI] + [(c, 5e-6) for c in br.CONV_BN] \
    + [(c, 2e-5) for c in br.BN if br.cfg_of(c)['relu'] and br.cfg_of(c)['res']] + [(c, _GN_TOL(c)) for c in br.GN] \
    + [(br.DCN[n], DCN_TOL) for n in ('xn', 'mm', 'mm_wg', 'grouped')] + [(br.PACK, 1e-5)]


@pytest.mark.parametrize('case,tol', SUNK_CASES, ids=[f'{c.op}-{c.name}' for c, _ in SUNK_CASES])
def test_parameter_gradients_onto_non_zero_sinks(case, tol):
    """conv2d, conv2d_multi, conv_bn_act (the single wgrad_bn), bn_act, GroupNorm.forward_multi / forward_cat_px, dcn_multi on
    the split ('xn', 'mm'), the matrix-pipe ('mm_wg') and the grouped weight-gradient kernel, and the DCNv2 pack, in 'bf16x6':
    base + gradient in the registered views, canaries and frozen views bit-identical, p.grad still the view."""
    with _math('bf16x6'):
        for state in SUNK_STATES:
            errs, _ = _run_sunk(case, state, tol)
            _line(f'sunk {state} {case.op} {case.name}', errs)


@pytest.mark.parametrize('variant', ['nchw_inputs', 'contiguous_weight'])
def test_dcn_sinks_declined_for_the_layout_take_the_classic_path(variant):
    """dcn_multi on 'xn' with sinks for w and b where the device backend declines them: inputs in contiguous (NCHW) memory, and
    channels-last inputs under a contiguous (not channels-last) weight parameter, which the backend re-lays into a temporary.
    Both gradients go back to autograd, whose AccumulateGrad adds them into the registered views: the leaf hooks see w and b,
    nobody is told `done`, p.grad is still the view, base + gradient within DCN_TOL, canaries bit-identical."""
    from lsnet_amd.ops import grad_sink
    case = br.DCN['xn']
    nhwc = variant == 'contiguous_weight'
    with _math('bf16x6'):
        ref = br.reference(case)
        leaves, t = _tensors(case, ref, br.leaf_names(case), nhwc)
        if nhwc:
            t['w'] = leaves['w'] = torch.nn.Parameter(leaves['w'].detach().contiguous())
        assert t['x'].is_contiguous(memory_format=_CL) == nhwc and not t['w'].is_contiguous(memory_format=_CL)
        params = collections.OrderedDict((n, leaves[n]) for n in ('w', 'b'))
        views, before, index = br.arena(params, ref.grads, seed=case.seed)
        done, returned = collections.Counter(), collections.Counter()
        for n, p in params.items():
            grad_sink.register(p, views[n], on_done=lambda p, n=n: done.update([n]))
            p.grad = views[n]
            p.register_hook(lambda g, n=n: returned.update([n] if g is not None else []))
        br.backward(br.dcn_outputs(case, t), _upstream(case, ref, nhwc), {})
        torch.cuda.synchronize()
        assert returned == collections.Counter(w=1, b=1) and not done, (returned, done)
        for n, p in params.items():
            assert p.grad is views[n] and p.grad.data_ptr() == views[n].data_ptr(), n
        errs = br.check_sunk(index['flat'], before, ref.grads, DCN_TOL, index)
        _line(f'sunk declined {variant} {case.op} {case.name}', errs)


@pytest.mark.parametrize('with_bias', [True, False])
def test_grouped_conv_weight_gradient_accumulates_at_the_c_entry(with_bias):
    """lsn_grouped_conv2d_backward_weight(accumulate = 1), which _GroupConvFn never passes: onto non-zero grad_w / grad_bias, and
    with grad_bias = NULL (the bias view then stays as it was)."""
    from lsnet_amd import _lib
    case = br.GCONV[0]
    c, ref = br.cfg_of(case), br.reference(case)
    x, w, go = _put(ref.leaves['x']), _put(ref.leaves['w']), _put(ref.gos[0])
    params = collections.OrderedDict(w=w, b=_put(ref.leaves['b']))
    views, before, index = br.arena(params, ref.grads, seed=case.seed)
    B, C, H, W = x.shape
    lib = _lib.load()
    _lib.check(lib.lsn_grouped_conv2d_backward_weight(x.data_ptr(), go.data_ptr(), views['w'].data_ptr(),
                                                      views['b'].data_ptr() if with_bias else None, B, H, W, C, C, c['k'], c['k'],
                                                      c['s'], c['p'], 1, c['G'], 1, _lib.stream()))
    torch.cuda.synchronize()
    errs = br.check_sunk(index['flat'], before, ref.grads, 2e-6, index, frozen=() if with_bias else ('b',))
    _line(f'sunk C entry gconv {case.name} bias {int(with_bias)}', errs)


# ================================================================================== C. one weight, two contributions
TWICE = [(br.CONV_MULTI[0], 3e-6, (2,)), (br.CONV_BN_PAIR, 5e-6, ()), (br.DCN_PAIR, DCN_TOL, ())]


def _conv_twice_outputs(case, t):
    """a Conv2d applied to two maps in two separate calls (CONV_MULTI[0] without its third map)"""
    from lsnet_amd.ops.conv import Conv2d
    c = br.cfg_of(case)
    m = Conv2d(c['C'], c['Co'], c['k'], padding=c['p'], bias=True).to(_dev())
    m.weight, m.bias = t['w'], t['b']
    return [m(t['x0']), m(t['x1']), m(t['x2']).detach()]


@pytest.mark.parametrize('case,tol,unused', TWICE, ids=[c.op for c, _, _ in TWICE])
def test_one_weight_two_contributions_plain_and_deferred(case, tol, unused):
    """A Conv2d, a conv_bn_act pair and a dcn_multi weight used twice in one backward, sinks on non-zero bases: base + g1 + g2
    when run plainly and between lsn_wgrad_defer(64) and lsn_wgrad_defer(0), where the second call finds a queued reduce for its
    gradient and has it run first (`clash`, csrc/conv.hip conv_wgrad_reduce) -- and the same bits both times, as the header
    promises (the same arithmetic per element in the same order).  (The conv_bn_act pair is what found the folded-norm reduce
    forming gw + a G as one fma in the deferred kernel and as a rounded product plus a sum in the immediate one: equal onto a
    zeroed bucket, 2961 of 18432 weight-gradient floats apart onto this base.)"""
    outputs = _conv_twice_outputs if case.op == 'conv2d_multi' else _outputs
    with _math('bf16x6'):
        errs, plain = _run_sunk(case, 'all_sunk', tol, unused, outputs, uses=2)
        _line(f'twice plain {case.op} {case.name}', errs)
        errs, deferred = _run_sunk(case, 'all_sunk', tol, unused, outputs, defer=True, uses=2)
        _line(f'twice deferred {case.op} {case.name}', errs)
        assert torch.equal(plain, deferred), int((plain != deferred).sum())
