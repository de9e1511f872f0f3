"""Requests, case tables, fp64 references and checks of the backward-request tests (tests/test_backward_requests_host.py,
tests/test_backward_requests_gpu.py).

Every backward entry point of the library takes optional outputs (a gradient that is not asked for is a NULL pointer) and
an `accumulate` flag (1: ADD the parameter gradient onto what the buffer holds).  The per-operator tests ask for every
gradient and hand over fresh buffers; the tables here vary both: WHICH leaves require a gradient (`requests`,
DCN_ROUTE_REQUESTS) and WHERE parameter gradients go (`arena`: gradient sinks on non-zero bases between canaries).

A case is (operator, name, cfg, seed).  `build` gives its leaves (the tensors a gradient can be asked for, by name), its
constants and one upstream gradient per output, all fp32 on the CPU from the case's own seed; `reference` evaluates the
operator ONCE in fp64 on the CPU (F.conv2d, F.batch_norm(training=False), F.group_norm, tests/torch_dcn_ref.py; the
deformable cases: the CPU oracle, which is what tests/test_ops_gpu.py test_dcn_forward_backward holds them to) with every
gradient requested -- a partial request must give the same numbers for what it asks and nothing for the rest.  With a ReLU
the upstream gradient goes through conv_geometry_cases.gate_safe, so every element can be held by the maximum.

No GPU import: the module serves the host test as it serves the device test."""
import collections

import torch
import torch.nn.functional as F

from tests.conv_geometry_cases import GATE_MARGIN, gate_safe, out_size, rel_diff  # noqa: F401  (re-exported)

GATE_SHARE_CAP = 0.05      # gate_safe may zero at most this share of an upstream gradient


# ---------------------------------------------------------------------------------- which gradients are asked for
def requests(leaves):
    """Every single leaf alone, every leave-one-out, all leaves; duplicates removed, each in the order of `leaves`.  For up
    to three leaves that is every non-empty subset."""
    leaves = tuple(leaves)
    out = []
    for r in [(l,) for l in leaves] + [tuple(m for m in leaves if m != l) for l in leaves] + [leaves]:
        if r and r not in out:
            out.append(r)
    return out


def subsets(leaves):
    """every non-empty subset of `leaves`, in the order of `leaves`"""
    leaves = tuple(leaves)
    return [tuple(l for i, l in enumerate(leaves) if m >> i & 1) for m in range(1, 1 << len(leaves))]


DCN_LEAVES = ('x', 'off', 'mask', 'w', 'b')

# name -> the request of ONE deformable level that takes the route (csrc/dcn_route.h route_backward, ops/hip_backend.py dcn_backward)
DCN_ROUTE_REQUESTS = collections.OrderedDict([
    ('weight_without_data', ('w',)),                 # any_data false: DATA_NONE, the weight gradient computes its own taps
    ('weight_bias_without_data', ('w', 'b')),        # the same with the bias sums in the launch
    ('bias_without_weight', ('b',)),                 # refused at the C entry: the backend asks for grad_weight and drops it
    ('input_alone', ('x',)),                         # the gather without corner products, WG_NONE
    ('offset_without_input', ('off',)),              # fails mm_bwd_ok / bwd_grouped_ok: the scatter kernels with gx == NULL
    ('offset_mask_without_input', ('off', 'mask')),
    ('mask_without_input', ('mask',)),
    ('data_without_params', ('x', 'off', 'mask')),   # the gather with corner products, WG_NONE
    ('input_and_weight', ('x', 'w')),                # the gather without corner products, its tap table read by the weight gradient
])

_has = lambda r, *names: all(n in r for n in names)
_none = lambda r, *names: not any(n in r for n in names)
# the Python statement of what each name claims about its request
DCN_ROUTE_PRECONDITIONS = {
    'weight_without_data': lambda r: _none(r, 'x', 'off', 'mask', 'b') and _has(r, 'w'),
    'weight_bias_without_data': lambda r: _none(r, 'x', 'off', 'mask') and _has(r, 'w', 'b'),
    'bias_without_weight': lambda r: _has(r, 'b') and _none(r, 'w'),
    'input_alone': lambda r: r == ('x',),
    'offset_without_input': lambda r: _has(r, 'off') and _none(r, 'x', 'mask'),     # some level has offset without input
    'offset_mask_without_input': lambda r: _has(r, 'off', 'mask') and _none(r, 'x'),
    'mask_without_input': lambda r: _has(r, 'mask') and _none(r, 'x', 'off'),
    'data_without_params': lambda r: _has(r, 'x', 'off', 'mask') and _none(r, 'w', 'b'),
    'input_and_weight': lambda r: _has(r, 'x', 'w') and _none(r, 'off', 'mask', 'b'),
}


def dcn_requests(case, everything=False):
    """The requests of a deformable case over the leaves it has: all non-empty subsets, or DCN_ROUTE_REQUESTS + all."""
    leaves = leaf_names(case)
    if everything:
        return subsets(leaves)
    out = []
    for r in list(DCN_ROUTE_REQUESTS.values()) + [leaves]:
        r = tuple(n for n in r if n in leaves)
        if r and r not in out:
            out.append(r)
    return out


# ---------------------------------------------------------------------------------- case tables
Case = collections.namedtuple('Case', 'op name cfg seed')
Built = collections.namedtuple('Built', 'leaves consts gos')            # leaves: OrderedDict name -> tensor; gos: one per output
Ref = collections.namedtuple('Ref', 'leaves consts gos ys grads gate_share')


def _case(op, name, seed, **cfg):
    return Case(op, name, tuple(sorted(cfg.items())), seed)


def cfg_of(case):
    return dict(case.cfg)


# conv2d (_ConvFn): a bias, a stride-2 case without one, Co % 4 with C <= 64 (the zero-filter padding of the data gradient)
CONV2D = [_case('conv2d', f'{n}{"_relu" if relu else ""}', 100 + 2 * i + relu, relu=relu, **kw)
          for i, (n, kw) in enumerate([('c32_co48_p1', dict(C=32, Co=48, k=3, s=1, p=1, H=9, W=11, bias=True)),
                                       ('c16_co32_s2', dict(C=16, Co=32, k=3, s=2, p=1, H=10, W=13, bias=False)),
                                       ('c32_co27', dict(C=32, Co=27, k=3, s=1, p=1, H=9, W=11, bias=True))])
          for relu in (False, True)]

# conv2d_multi (_ConvMultiFn): three maps under one weight, with and without residuals and ReLU
_SIZES3 = ((9, 7), (5, 4), (1, 1))
CONV_MULTI = [_case('conv2d_multi', f'res{int(res)}_relu{int(relu)}', 200 + 2 * res + relu, C=32, Co=32, k=3, p=1, sizes=_SIZES3,
                    res=res, relu=relu) for res in (False, True) for relu in (False, True)]


def conv_multi_requests(case):
    """need_x patterns TFT, FFF (with the parameters), TTT; w only; b only; one residual only; all"""
    res = cfg_of(case)['res']
    reqs = [('x0', 'x2'), ('w', 'b'), ('x0', 'x1', 'x2'), ('w',), ('b',)]
    if res:
        reqs.append(('r1',))
    return reqs + [leaf_names(case)]


# grouped convolution (_GroupConvFn)
GCONV = [_case('gconv', 'c32_g8', 300, C=32, G=8, k=3, s=1, p=1, H=9, W=11, bias=True),
         _case('gconv', 'c64_g2_s2', 301, C=64, G=2, k=3, s=2, p=1, H=9, W=11, bias=False)]

# conv_bn_act (_ConvBnActFn); gamma holds a 0 and a 1e-6 channel as in test_conv_bn_act_folded
CONV_BN = [_case('conv_bn_act', 'k3_s1_res_relu', 400, C=32, Co=64, k=3, s=1, p=1, H=9, W=11, res=True, relu=True),
           _case('conv_bn_act', 'k1_s2', 401, C=32, Co=64, k=1, s=2, p=0, H=9, W=11, res=False, relu=False)]

# bn_act (_BnActFn): C2048 = two 1024-channel slices, C4 at one pixel = 256 row slots for one row
BN = [_case('bn_act', f'c{C}_{B}x{H}x{W}_relu{int(relu)}_res{int(res)}', 500 + 4 * i + 2 * relu + res, C=C, B=B, H=H, W=W,
            relu=relu, res=res)
      for i, (C, B, H, W) in enumerate([(64, 2, 3, 5), (2048, 2, 3, 5), (4, 1, 1, 1)])
      for relu in (False, True) for res in (False, True)]

# GroupNorm.forward_multi / forward_cat_px: four and two channels per group (the element-group kernels)
GN = [_case('gn', f'c{C}_g8_relu{int(relu)}_{"cat" if cat else "multi"}', 600 + 8 * i + 2 * relu + cat, C=C, G=8,
            sizes=((9, 7), (3, 2)), relu=relu, cat=cat)
      for i, C in enumerate((32, 16)) for relu in (False, True) for cat in (False, True)]
GN_REQUESTS = [('x0',), ('x1',), ('gamma',), ('beta',), ('gamma', 'beta'), ('x0', 'x1'), ('x0', 'x1', 'gamma', 'beta')]

# dcn_multi (_DCNFunction): 3x3, pad 1, offsets rand * 6 - 3 as tests/test_ops_gpu.py _make
DCN = collections.OrderedDict((c.name, c) for c in [
    _case('dcn', 'xn', 700, C=16, Co=24, groups=1, hw=(7, 9), mask=True, bias=True),
    _case('dcn', 'mm', 701, C=64, Co=128, groups=1, hw=(6, 10), mask=True, bias=True),
    # (the matrix-pipe WEIGHT gradient wants Co % 256 == 0, csrc/dcn.hip mm_wgrad_ok: 'mm' takes the matrix pipe for its data
    # gradient and the split kernel for its weight gradient, this one the matrix pipe for both)
    _case('dcn', 'mm_wg', 702, C=64, Co=256, groups=1, hw=(6, 10), mask=True, bias=True),
    _case('dcn', 'grouped', 703, C=64, Co=64, groups=4, hw=(7, 9), mask=True, bias=True),
    _case('dcn', 'v1', 704, C=32, Co=48, groups=1, hw=(7, 9), mask=False, bias=False),
])
# one PyramidDeformConv-style call: (source, offset grid) per level; source A is shared by levels 0 and 2
DCN_PYR = _case('dcn_pyr', 'pyr', 710, C=32, Co=32, src=(('A', (5, 7)), ('B', (9, 13))),
                levels=(('A', (9, 13)), ('B', (5, 7)), ('A', (5, 7))))
PYR_REQUESTS = [('xA',), ('xB',), ('xA', 'off0', 'off1', 'off2'), ('xB', 'off0'), ('xA', 'w'), ('xB', 'off0', 'off1', 'off2', 'w'),
                ('off0',), ('off0', 'off1', 'off2', 'w'), ('w',), ('xA', 'xB', 'off0', 'off1', 'off2', 'w')]

# ModulatedDeformConvPack.forward_multi (_DCNPackFn)
PACK = _case('pack', 'c32_co32', 800, C=32, Co=32, sizes=((9, 7), (5, 4)))
PACK_REQUESTS = [('weight', 'bias', 'w_off', 'b_off'),      # x frozen, every parameter trainable
                 ('w_off', 'b_off'), ('weight',), ('x0', 'x1'), ('x0', 'x1', 'weight', 'bias', 'w_off', 'b_off')]

# one weight under two separate calls of one graph (its gradient has two contributions): a Conv2d is CONV_MULTI[0] with its third
# map left out of the loss; a conv_bn_act pair and a dcn_multi weight at the channel counts of 'xn' get cases of their own
CONV_BN_PAIR = _case('conv_bn_pair', 'k3_relu', 900, C=32, Co=64, k=3, s=1, p=1, sizes=((9, 7), (5, 4)), relu=True)
DCN_PAIR = _case('dcn_pair', 'xn_twice', 901, C=16, Co=24, sizes=((7, 9), (5, 6)))

ALL = CONV2D + CONV_MULTI + GCONV + CONV_BN + BN + GN + list(DCN.values()) + [DCN_PYR, PACK, CONV_BN_PAIR, DCN_PAIR]

PARAMS = {'conv2d': ('w', 'b'), 'conv2d_multi': ('w', 'b'), 'gconv': ('w', 'b'), 'conv_bn_act': ('w', 'gamma', 'beta'),
          'bn_act': ('gamma', 'beta'), 'gn': ('gamma', 'beta'), 'dcn': ('w', 'b'), 'dcn_pyr': ('w',),
          'pack': ('weight', 'bias', 'w_off', 'b_off'), 'conv_bn_pair': ('w', 'gamma', 'beta'), 'dcn_pair': ('w', 'b')}


def param_names(case):
    return tuple(n for n in leaf_names(case) if n in PARAMS[case.op])


# ---------------------------------------------------------------------------------- seeded inputs
def _bn_consts(g, C):
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[0], gamma[1] = 0.0, 1e-6
    if C > 8:
        gamma[8:12] *= -1.0
    return gamma, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5


def build(case):
    """(leaves, consts, gos): fp32 CPU tensors from the case's own seed, weights scaled for outputs of order one"""
    c, g = cfg_of(case), torch.Generator().manual_seed(case.seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    L, K = collections.OrderedDict(), {}
    B = 2
    if case.op == 'conv2d':
        L['x'], L['w'] = rn(B, c['C'], c['H'], c['W']), rn(c['Co'], c['C'], c['k'], c['k']) / (c['C'] * c['k'] ** 2) ** 0.5
        if c['bias']:
            L['b'] = rn(c['Co'])
        shapes = [(B, c['Co'], out_size(c['H'], c['k'], c['s'], c['p'], 1), out_size(c['W'], c['k'], c['s'], c['p'], 1))]
    elif case.op == 'conv2d_multi':
        for i, (h, w) in enumerate(c['sizes']):
            L[f'x{i}'] = rn(B, c['C'], h, w)
        L['w'], L['b'] = rn(c['Co'], c['C'], c['k'], c['k']) / (c['C'] * c['k'] ** 2) ** 0.5, rn(c['Co'])
        shapes = [(B, c['Co'], h, w) for h, w in c['sizes']]
        if c['res']:
            for i, s in enumerate(shapes):
                L[f'r{i}'] = rn(*s)
    elif case.op == 'gconv':
        cg = c['C'] // c['G']
        L['x'], L['w'] = rn(B, c['C'], c['H'], c['W']), rn(c['C'], cg, c['k'], c['k']) / (cg * c['k'] ** 2) ** 0.5
        if c['bias']:
            L['b'] = rn(c['C'])
        shapes = [(B, c['C'], out_size(c['H'], c['k'], c['s'], c['p'], 1), out_size(c['W'], c['k'], c['s'], c['p'], 1))]
    elif case.op == 'conv_bn_act':
        L['x'], L['w'] = rn(B, c['C'], c['H'], c['W']), rn(c['Co'], c['C'], c['k'], c['k']) / (c['C'] * c['k'] ** 2) ** 0.5
        L['gamma'], L['beta'], K['mean'], K['var'] = _bn_consts(g, c['Co'])
        shapes = [(B, c['Co'], out_size(c['H'], c['k'], c['s'], c['p'], 1), out_size(c['W'], c['k'], c['s'], c['p'], 1))]
        if c['res']:
            L['residual'] = rn(*shapes[0])
    elif case.op == 'bn_act':
        shapes = [(c['B'], c['C'], c['H'], c['W'])]
        L['x'] = rn(*shapes[0])
        if c['res']:
            L['residual'] = rn(*shapes[0])
        L['gamma'], L['beta'] = rn(c['C']) * 0.5 + 1, rn(c['C']) * 0.2
        K['mean'], K['var'] = rn(c['C']), torch.rand(c['C'], generator=g) + 0.3
    elif case.op == 'gn':
        shapes = [(B, c['C'], h, w) for h, w in c['sizes']]
        for i, s in enumerate(shapes):   # channels of different scale and mean: the statistics are not those of a unit normal
            L[f'x{i}'] = rn(*s) * (0.5 + 2 * torch.rand(1, c['C'], 1, 1, generator=g)) + 2 * rn(1, c['C'], 1, 1)
        L['gamma'], L['beta'] = rn(c['C']) * 0.5 + 1, rn(c['C']) * 0.3
    elif case.op == 'dcn':
        (H, W), cg = c['hw'], c['C'] // c['groups']
        L['x'] = rn(B, c['C'], H, W)
        L['off'] = torch.rand(B, 18, H, W, generator=g) * 6 - 3       # reaches outside the map
        if c['mask']:
            L['mask'] = torch.rand(B, 9, H, W, generator=g)
        L['w'] = rn(c['Co'], cg, 3, 3) / (3 * cg ** 0.5)
        if c['bias']:
            L['b'] = rn(c['Co'])
        shapes = [(B, c['Co'], H, W)]
    elif case.op == 'dcn_pyr':
        for n, (h, w) in c['src']:
            L[f'x{n}'] = rn(B, c['C'], h, w)
        for i, (_, (h, w)) in enumerate(c['levels']):
            L[f'off{i}'] = torch.rand(B, 18, h, w, generator=g) * 6 - 3
        L['w'] = rn(c['Co'], c['C'], 3, 3) / (3 * c['C'] ** 0.5)
        shapes = [(B, c['Co'], h, w) for _, (h, w) in c['levels']]
    elif case.op == 'conv_bn_pair':
        for i, (h, w) in enumerate(c['sizes']):
            L[f'x{i}'] = rn(B, c['C'], h, w)
        L['w'] = rn(c['Co'], c['C'], c['k'], c['k']) / (c['C'] * c['k'] ** 2) ** 0.5
        L['gamma'], L['beta'], K['mean'], K['var'] = _bn_consts(g, c['Co'])
        shapes = [(B, c['Co'], h, w) for h, w in c['sizes']]
    elif case.op == 'dcn_pair':
        for i, (h, w) in enumerate(c['sizes']):
            L[f'x{i}'], L[f'off{i}'] = rn(B, c['C'], h, w), torch.rand(B, 18, h, w, generator=g) * 6 - 3
            L[f'mask{i}'] = torch.rand(B, 9, h, w, generator=g)
        L['w'], L['b'] = rn(c['Co'], c['C'], 3, 3) / (3 * c['C'] ** 0.5), rn(c['Co'])
        shapes = [(B, c['Co'], h, w) for h, w in c['sizes']]
    elif case.op == 'pack':
        for i, (h, w) in enumerate(c['sizes']):
            L[f'x{i}'] = rn(B, c['C'], h, w)
        L['weight'], L['bias'] = rn(c['Co'], c['C'], 3, 3) / (3 * c['C'] ** 0.5), rn(c['Co'])
        L['w_off'], L['b_off'] = rn(27, c['C'], 3, 3) * 0.05, rn(27) * 0.5    # as test_dcn_pack_fused_offset_mask_logits
        shapes = [(B, c['Co'], h, w) for h, w in c['sizes']]
    else:
        raise KeyError(case.op)
    return Built(L, K, [rn(*s) for s in shapes])


def leaf_names(case):
    return tuple(build(case).leaves)


def pyr_scales(case):
    """per level (scale_h, scale_w) = source size / offset grid, as LSHead rescales a neighbour level's positions"""
    c = cfg_of(case)
    src = dict(c['src'])
    return [(src[n][0] / h, src[n][1] / w) for n, (h, w) in c['levels']]


# ---------------------------------------------------------------------------------- the operators in torch
BN_EPS = GN_EPS = 1e-5


def pre_activations(case, t):
    """The operator on the tensors `t` (leaves and constants by name, any dtype) in plain torch -> one tensor per output, in
    front of the ReLU where the case has one"""
    c = cfg_of(case)
    if case.op == 'conv2d':
        return [F.conv2d(t['x'], t['w'], t.get('b'), c['s'], c['p'])]
    if case.op == 'conv2d_multi':
        ys = [F.conv2d(t[f'x{i}'], t['w'], t['b'], 1, c['p']) for i in range(len(c['sizes']))]
        return [y + t[f'r{i}'] for i, y in enumerate(ys)] if c['res'] else ys
    if case.op == 'gconv':
        return [F.conv2d(t['x'], t['w'], t.get('b'), c['s'], c['p'], 1, c['G'])]
    if case.op == 'conv_bn_act':
        z = F.batch_norm(F.conv2d(t['x'], t['w'], None, c['s'], c['p']), t['mean'], t['var'], t['gamma'], t['beta'], False, 0.0, BN_EPS)
        return [z + t['residual'] if c['res'] else z]
    if case.op == 'conv_bn_pair':
        return [F.batch_norm(F.conv2d(t[f'x{i}'], t['w'], None, c['s'], c['p']), t['mean'], t['var'], t['gamma'], t['beta'], False,
                             0.0, BN_EPS) for i in range(len(c['sizes']))]
    if case.op == 'bn_act':
        z = F.batch_norm(t['x'], t['mean'], t['var'], t['gamma'], t['beta'], False, 0.0, BN_EPS)
        return [z + t['residual'] if c['res'] else z]
    if case.op == 'gn':
        return [F.group_norm(t[f'x{i}'], c['G'], t['gamma'], t['beta'], GN_EPS) for i in range(len(c['sizes']))]
    if case.op == 'pack':
        from tests.torch_dcn_ref import torch_dcn
        ys = []
        for i in range(len(c['sizes'])):
            om = F.conv2d(t[f'x{i}'], t['w_off'], t['b_off'], 1, 1)
            ys.append(torch_dcn(t[f'x{i}'], om[:, :18], torch.sigmoid(om[:, 18:]), t['weight'], t['bias'], 1, 1, 1, 1, 1))
        return ys
    raise KeyError(case.op)


def _relu(case):
    return bool(cfg_of(case).get('relu'))


def _autograd_reference(case, b, unused, dtype):
    t = {n: v.to(dtype) for n, v in b.consts.items()}
    leaves = collections.OrderedDict((n, v.to(dtype).requires_grad_()) for n, v in b.leaves.items())
    t.update(leaves)
    pre = pre_activations(case, t)
    gos, shares = [], []
    for i, (p, go) in enumerate(zip(pre, b.gos)):
        if i in unused:
            gos.append(None)
            continue
        if _relu(case):
            safe = gate_safe(p.detach().double(), go.double()).float()
            shares.append(float((safe == 0).double().mean() - (go == 0).double().mean()))
            go = safe
        gos.append(go)
    ys = [F.relu(p) if _relu(case) else p for p in pre]
    used = [i for i in range(len(ys)) if i not in unused]
    grads = torch.autograd.grad([ys[i] for i in used], list(leaves.values()), [gos[i].to(dtype) for i in used], allow_unused=True)
    grads = collections.OrderedDict((n, torch.zeros_like(v) if g is None else g) for (n, v), g in zip(leaves.items(), grads))
    return gos, [y.detach() for y in ys], grads, max(shares, default=0.0)


def _oracle_reference(case, b, unused):
    """the deformable cases: tests/test_ops_gpu.py holds them to the CPU oracle (fp32 C, its own summation order)"""
    from oracle import oracle_py as orc
    c, L = cfg_of(case), b.leaves
    if case.op == 'dcn':
        levels, scales, groups = [('x', 'off', 'mask' if c['mask'] else None)], [(1.0, 1.0)], c['groups']
    elif case.op == 'dcn_pair':
        levels, scales, groups = [(f'x{i}', f'off{i}', f'mask{i}') for i in range(len(c['sizes']))], [(1.0, 1.0)] * len(c['sizes']), 1
    else:
        levels, scales, groups = [(f'x{n}', f'off{i}', None) for i, (n, _) in enumerate(c['levels'])], pyr_scales(case), 1
    grads = collections.OrderedDict((n, torch.zeros_like(v).double()) for n, v in L.items())
    ys, gos = [], []
    for i, ((xn, on, mn), (sh, sw)) in enumerate(zip(levels, scales)):
        x, off, mask = L[xn], L[on], (L[mn] if mn else None)
        ys.append(orc.deform_conv_forward(x, L['w'], L.get('b'), off, mask, 1, 1, 1, groups, 1, sh, sw, out_hw=tuple(off.shape[2:])).double())
        gos.append(None if i in unused else b.gos[i])
        if i in unused:
            continue
        g = orc.deform_conv_backward(x, L['w'], off, mask, b.gos[i], 1, 1, 1, groups, 1, sh, sw)
        grads[xn] += g['gx'].double()
        grads[on] += g['goff'].double()
        grads['w'] += g['gw'].double()
        if mn:
            grads[mn] += g['gmask'].double()
        if 'b' in L:
            grads['b'] += g['gb'].double()
    return gos, ys, grads, 0.0


_refs = {}


def reference(case, unused=()):
    """The shared reference of a case, computed once: leaves, constants, the upstream gradients as the backward pass gets them
    (gated; None for an output in `unused`, which stays out of the loss), outputs and the gradient of EVERY leaf."""
    key = (case, tuple(sorted(unused)))
    if key not in _refs:
        b = build(case)
        if case.op in ('dcn', 'dcn_pyr', 'dcn_pair'):
            gos, ys, grads, share = _oracle_reference(case, b, key[1])
        else:
            gos, ys, grads, share = _autograd_reference(case, b, key[1], torch.float64)
        _refs[key] = Ref(b.leaves, b.consts, gos, ys, grads, share)
    return _refs[key]


def aten_fp32_error(case):
    """max over the gradients of rel_diff(ATen fp32 on the CPU, fp64): what fp32 arithmetic alone costs on this case"""
    ref = reference(case)
    b = Built(ref.leaves, ref.consts, [g for g in ref.gos])
    t = {n: v.float() for n, v in b.consts.items()}
    leaves = collections.OrderedDict((n, v.float().requires_grad_()) for n, v in b.leaves.items())
    t.update(leaves)
    pre = pre_activations(case, t)
    ys = [F.relu(p) if _relu(case) else p for p in pre]
    grads = torch.autograd.grad(ys, list(leaves.values()), [g.float() for g in ref.gos])
    return {n: rel_diff(g.double(), ref.grads[n]) for n, g in zip(leaves, grads)}


# ---------------------------------------------------------------------------------- running a request
def dcn_outputs(case, t):
    """ops.dcn_multi on the tensors `t` of a deformable case (whatever backend serves their device) -> one output per level"""
    from lsnet_amd import ops
    c = cfg_of(case)
    if case.op == 'dcn':
        return ops.dcn_multi([t['x']], [t['off']], [t.get('mask')], t['w'], t.get('b'), 1, 1, 1, c['groups'], 1)
    if case.op == 'dcn_pair':      # two calls: the weight is used twice in one graph
        return [ops.dcn_multi([t[f'x{i}']], [t[f'off{i}']], [t[f'mask{i}']], t['w'], t['b'], 1, 1, 1)[0] for i in range(len(c['sizes']))]
    return ops.dcn_multi([t[f'x{n}'] for n, _ in c['levels']], [t[f'off{i}'] for i in range(len(c['levels']))], None, t['w'], None,
                         1, 1, 1, 1, 1, scales=pyr_scales(case), pyramid=True)


def backward(outs, gos, leaves):
    """.backward() of the outputs under their upstream gradients (None: the output stays out of the loss), as a training step
    runs it -> name -> the leaf's .grad"""
    used = [(o, g) for o, g in zip(outs, gos) if g is not None]
    torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    return {n: t.grad for n, t in leaves.items()}


# ---------------------------------------------------------------------------------- checks
def check_request(got, want, requested, tol):
    """got: name -> the leaf's .grad after backward (None: none came).  Every requested gradient within `tol` of the range of
    its reference (tests/test_ops_gpu.py _err), every other leaf without one.  Returns name -> error."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    errs = {}
    for n, r in want.items():
        g = got[n]
        if n not in requested:
            assert g is None, f'{n}: a gradient came back that was not asked for (request {requested})'
            continue
        assert g is not None, f'{n}: no gradient came back (request {requested})'
        assert tuple(g.shape) == tuple(r.shape), (n, tuple(g.shape), tuple(r.shape))
        errs[n] = rel_diff(g.detach().double().cpu(), r)
        assert errs[n] < tol_of(tol, n), f'{n}: {errs[n]:.3e} >= {tol_of(tol, n):.1e} (request {requested})'
    return errs


def tol_of(tol, name):
    """a tolerance for all gradients, or name -> tolerance with the entry None for the names it does not list"""
    return tol.get(name, tol.get(None)) if isinstance(tol, dict) else tol


ADD_ROUNDING = 2.0 ** -22    # (one fp32 add of two values no larger than the range costs at most 2^-23 of it)


def arena(params, refs, gap=64, seed=0):
    """One flat fp32 tensor (on the parameters' device) with a view per parameter -- the parameter's shape and strides, 16-byte
    aligned -- between runs of `gap` canary floats.  The views hold `base` values: randn, cut at one sigma, times the range of
    the parameter's fp64 reference gradient (from the reference, never from the device), so that neither term of base +
    gradient exceeds the range.  params / refs: name -> tensor.  Returns (views by name, a clone of the whole arena, index):
    index['flat'] is the arena, index['canary'] the positions of the canary floats, index['slots'] name -> (offset, numel)."""
    assert gap % 4 == 0
    g = torch.Generator().manual_seed(seed)
    slots, pieces, canary, o = {}, [], [], 0

    def run_of_canaries():
        nonlocal o
        pieces.append(torch.randn(gap, generator=g) * 1e3)
        canary.extend(range(o, o + gap))
        o += gap

    run_of_canaries()
    for n, p in params.items():
        numel = p.numel()
        scale = max(float(refs[n].abs().max()), 1e-30)
        pieces.append(torch.randn(numel, generator=g).clamp(-1, 1) * scale)
        slots[n] = (o, numel)
        o += numel
        pad = -o % 4
        if pad:
            pieces.append(torch.randn(pad, generator=g) * 1e3)
            canary.extend(range(o, o + pad))
            o += pad
        run_of_canaries()
    dev = next(iter(params.values())).device
    flat = torch.cat(pieces).to(dev)
    views = {}
    for n, p in params.items():
        views[n] = flat.as_strided(tuple(p.shape), p.stride(), slots[n][0])
        assert views[n].data_ptr() % 16 == 0 or flat.data_ptr() % 16
    index = dict(flat=flat, canary=torch.tensor(canary, dtype=torch.long, device=dev), slots=slots,
                 shapes={n: (tuple(p.shape), p.stride()) for n, p in params.items()})
    return views, flat.clone(), index


def _view(flat, index, n):
    shape, stride = index['shapes'][n]
    return flat.as_strided(shape, stride, index['slots'][n][0])


def check_sunk(arena_after, arena_before, refs, tol, index, frozen=()):
    """view == base + reference within tol + 2^-22 of the reference's range for every parameter of `refs` not in `frozen`;
    canaries and the views of frozen parameters bit-identical.  Returns name -> error."""
    ca, cb = arena_after[index['canary']], arena_before[index['canary']]
    assert torch.equal(ca, cb), f'{int((ca != cb).sum())} canary floats between the gradient views were written'
    errs = {}
    for n in index['slots']:
        after, before = _view(arena_after, index, n), _view(arena_before, index, n)
        if n in frozen:
            assert torch.equal(after, before), f'{n}: the view of a frozen parameter was written'
            continue
        want = before.detach().double().cpu() + refs[n]
        errs[n] = float((after.detach().double().cpu() - want).abs().max()) / max(float(refs[n].abs().max()), 1e-12)
        assert errs[n] < tol_of(tol, n) + ADD_ROUNDING, f'{n}: {errs[n]:.3e} >= {tol_of(tol, n) + ADD_ROUNDING:.1e} off base + gradient'
    return errs


MISTAKES = ('overwrite', 'added_twice', 'frozen_written', 'neighbour_written', 'bias_from_weight_only_call_missing',
            'unrequested_returned')


def mistaken(kind, base, ref):
    """What a plausible calling-convention mistake leaves where the right value is base + ref (sinks) or ref (returned
    gradients): torch models, applied by tests/test_backward_requests_host.py to the place the kind is about."""
    ref = ref.to(base.dtype)
    if kind == 'overwrite':              # accumulate = 0 on a sink: sink = g
        return ref.clone()
    if kind == 'added_twice':            # the kernel accumulated AND autograd added the returned gradient
        return base + 2 * ref
    if kind == 'frozen_written':         # a frozen parameter's view got its gradient all the same
        return base + ref
    if kind == 'neighbour_written':      # base: canary floats; one of them changed
        out = base.clone()
        out.view(-1)[out.numel() // 2] += 1.0
        return out
    if kind == 'bias_from_weight_only_call_missing':     # the weight-only workaround forgot the bias sums: zeros
        return torch.zeros_like(ref)
    if kind == 'unrequested_returned':   # a gradient nobody asked for (the right one, even)
        return ref.clone()
    raise KeyError(kind)
