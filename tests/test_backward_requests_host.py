"""tests/backward_request_cases.py checked on the CPU, and the wrapper logic of ops/dcn.py behind the CPU oracle.

What the device test (tests/test_backward_requests_gpu.py) leans on is held here first: `requests` yields the sets it says,
every DCN_ROUTE_REQUESTS entry meets the precondition of the route it is named for, gate_safe removes at most 5 % of an
upstream gradient, and check_request / check_sunk accept the reference and reject every calling-convention mistake of
`mistaken`.  Then `_DCNFunction` itself -- which gradients it asks its backend for and which it hands back -- with the oracle as
the backend: partial requests on one level, on a pyramid call with a shared and a detached source, on the fused-logits form,
and parameters whose .grad is a registered sink (the oracle backend has no sink support: the classic path must still ADD
into the registered view)."""
import collections

import pytest
import torch

from tests import backward_request_cases as br

ORACLE_TOL = 1e-6       # the same oracle on the same tensors; autograd's sum of a shared source's two gradients is fp32


def test_requests_yield_the_expected_sets():
    assert br.requests('a') == [('a',)]
    assert br.requests('ab') == [('a',), ('b',), ('a', 'b')]
    for leaves in ('ab', 'abc'):        # up to three leaves: every non-empty subset
        assert sorted(br.requests(leaves)) == sorted(br.subsets(leaves))
    r5 = br.requests(br.DCN_LEAVES)
    assert len(r5) == len(set(r5)) == 11 and len(br.subsets(br.DCN_LEAVES)) == 31
    assert [r for r in r5 if len(r) == 1] == [(l,) for l in br.DCN_LEAVES]
    assert sorted(r for r in r5 if len(r) == 4) == sorted(tuple(m for m in br.DCN_LEAVES if m != l) for l in br.DCN_LEAVES)
    assert r5[-1] == br.DCN_LEAVES
    assert all(r == tuple(l for l in br.DCN_LEAVES if l in r) for r in r5)


def test_route_requests_meet_their_preconditions():
    assert len(br.DCN_ROUTE_REQUESTS) == 9 and len(set(br.DCN_ROUTE_REQUESTS.values())) == 9
    assert set(br.DCN_ROUTE_REQUESTS) == set(br.DCN_ROUTE_PRECONDITIONS)
    assert set(br.DCN_ROUTE_REQUESTS.values()) == {('w',), ('w', 'b'), ('b',), ('x',), ('off',), ('off', 'mask'), ('mask',),
                                                    ('x', 'off', 'mask'), ('x', 'w')}
    for name, req in br.DCN_ROUTE_REQUESTS.items():
        assert set(req) <= set(br.DCN_LEAVES)
        assert br.DCN_ROUTE_PRECONDITIONS[name](req), name
        # ... and no other entry's: each request separates ONE route
        assert [n for n, ok in br.DCN_ROUTE_PRECONDITIONS.items() if ok(req)] == [name], name
    # a case without mask and bias keeps the distinct remainders, the full request last
    v1 = br.dcn_requests(br.DCN['v1'])
    assert v1 == [('w',), ('x',), ('off',), ('x', 'off'), ('x', 'w'), ('x', 'off', 'w')]
    assert len(br.dcn_requests(br.DCN['xn'])) == 10 and len(br.dcn_requests(br.DCN['xn'], everything=True)) == 31


def test_case_tables():
    assert len({(c.op, c.name) for c in br.ALL}) == len(br.ALL) and len({c.seed for c in br.ALL}) == len(br.ALL)
    for c in br.ALL:
        names = br.leaf_names(c)
        assert set(br.param_names(c)) <= set(names) and len(names) > len(br.param_names(c))
    for c in br.CONV_MULTI:
        assert all(set(r) <= set(br.leaf_names(c)) for r in br.conv_multi_requests(c))
    assert all(set(r) <= set(br.leaf_names(br.DCN_PYR)) for r in br.PYR_REQUESTS)
    assert all(set(r) <= set(br.leaf_names(br.PACK)) for r in br.PACK_REQUESTS)
    # the pyramid case: source A under two levels, B under one; requests with A and without B and the reverse
    lv = [n for n, _ in br.cfg_of(br.DCN_PYR)['levels']]
    assert lv.count('A') == 2 and lv.count('B') == 1
    assert any('xA' in r and 'xB' not in r for r in br.PYR_REQUESTS) and any('xB' in r and 'xA' not in r for r in br.PYR_REQUESTS)
    # the zero-filter padding of the data gradient: Co % 4 and C <= 64
    assert any(br.cfg_of(c)['Co'] % 4 and br.cfg_of(c)['C'] <= 64 for c in br.CONV2D)
    # the folded norm's gamma holds a zero and a 1e-6 channel
    for c in br.CONV_BN:
        gamma = br.build(c).leaves['gamma']
        assert gamma[0] == 0 and gamma[1] == pytest.approx(1e-6) and (gamma < 0).any()


@pytest.mark.parametrize('c', br.ALL, ids=[f'{c.op}-{c.name}' for c in br.ALL])
def test_reference_and_gate_share(c):
    """The fp64 reference has a finite, non-zero gradient for every leaf, and gate_safe zeroes at most 5 % of any upstream
    gradient (asserted on the reference alone; measured 0.2 % to 1.2 %)."""
    ref = br.reference(c)
    for n, g in ref.grads.items():
        assert g.shape == ref.leaves[n].shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    assert 0.0 <= ref.gate_share <= br.GATE_SHARE_CAP, ref.gate_share
    if br.cfg_of(c).get('relu'):
        if sum(y.numel() for y in ref.ys) >= 1000:
            assert ref.gate_share > 0       # the margin is live: some gate does lie within 1e-3 of zero
        pre =br.pre_activations(c, {n: v.double() for n, v in list(ref.leaves.items()) + list(ref.consts.items())})
        for p, go in zip(pre, ref.gos):
            near = p.abs() <= br.GATE_MARGIN * p.abs().max()
            assert (go[near] == 0).all()


def test_an_unused_output_has_its_own_reference():
    c = br.CONV_MULTI[0]
    full, part = br.reference(c), br.reference(c, unused=(1,))
    assert part.gos[1] is None and float(part.grads['x1'].abs().max()) == 0
    assert torch.equal(part.grads['x0'], full.grads['x0']) and br.rel_diff(part.grads['w'], full.grads['w']) > 1e-3


# ---------------------------------------------------------------------------------- the checks reject the mistakes
def _as_got(ref, requested):
    return {n: (g.float() if n in requested else None) for n, g in ref.grads.items()}


def test_check_request_accepts_the_reference_and_rejects_the_mistakes():
    ref = br.reference(br.DCN['xn'])
    for req in br.dcn_requests(br.DCN['xn'], everything=True):
        errs = br.check_request(_as_got(ref, req), ref.grads, req, 1e-6)
        assert set(errs) == set(req)
    # the weight-only workaround forgot the bias sums
    got = _as_got(ref, ('b',))
    got['b'] = br.mistaken('bias_from_weight_only_call_missing', got['b'], ref.grads['b'])
    with pytest.raises(AssertionError, match='b: '):
        br.check_request(got, ref.grads, ('b',), 1e-4)
    # the weight gradient the workaround asked for comes back although nobody wanted it
    got = _as_got(ref, ('b',))
    got['w'] = br.mistaken('unrequested_returned', ref.grads['w'].float(), ref.grads['w'])
    with pytest.raises(AssertionError, match='not asked for'):
        br.check_request(got, ref.grads, ('b',), 1e-4)
    # a requested gradient that never came, and one that is off by a part in a thousand
    got = _as_got(ref, ('x', 'w'))
    got['w'] = None
    with pytest.raises(AssertionError, match='no gradient came back'):
        br.check_request(got, ref.grads, ('x', 'w'), 1e-4)
    got = _as_got(ref, ('x', 'w'))
    got['x'] = got['x'] * 1.001
    with pytest.raises(AssertionError, match='x: '):
        br.check_request(got, ref.grads, ('x', 'w'), 1e-4)


def _arena_for(case, names):
    ref = br.reference(case)
    params = collections.OrderedDict((n, ref.leaves[n].clone()) for n in names)
    params['w'] = params['w'].contiguous(memory_format=torch.channels_last)       # a view with the parameter's own strides
    views, before, index = br.arena(params, ref.grads, seed=case.seed)
    return ref, params, views, before, index


def test_arena_layout():
    ref, params, views, before, index = _arena_for(br.DCN['xn'], ('w', 'b'))
    flat = index['flat']
    assert flat.dtype == torch.float32 and flat.dim() == 1
    for n, p in params.items():
        v = views[n]
        assert v.shape == p.shape and v.stride() == p.stride() and v.data_ptr() % 16 == flat.data_ptr() % 16
        assert float(v.abs().max()) <= float(ref.grads[n].abs().max())       # base values inside the reference's range
        assert float(v.abs().max()) > 0.5 * float(ref.grads[n].abs().max())
        o, numel = index['slots'][n]
        assert o % 4 == 0 and o >= 64 and not set(range(o, o + numel)) & set(index['canary'].tolist())
    assert len(index['canary']) >= 3 * 64 and torch.equal(flat, before) and flat.data_ptr() != before.data_ptr()
    assert len(index['canary']) + sum(k for _, k in index['slots'].values()) == flat.numel()


def test_check_sunk_accepts_the_reference_and_rejects_the_mistakes():
    ref, params, views, before, index = _arena_for(br.DCN['xn'], ('w', 'b'))
    flat = index['flat']

    def reset():
        flat.copy_(before)

    def put(n, value):
        views[n].copy_(value)

    base = {n: v.clone() for n, v in views.items()}
    right = {n: (base[n].double() + ref.grads[n]).float() for n in views}
    for n in views:
        put(n, right[n])
    errs = br.check_sunk(flat, before, ref.grads, 1e-6, index)
    assert set(errs) == {'w', 'b'} and max(errs.values()) <= br.ADD_ROUNDING
    for kind in ('overwrite', 'added_twice'):
        for n in views:
            reset()
            put('w', right['w']), put('b', right['b'])
            put(n, br.mistaken(kind, base[n], ref.grads[n]))
            with pytest.raises(AssertionError, match=f'{n}: '):
                br.check_sunk(flat, before, ref.grads, 1e-4, index)
    # frozen: the bias view must not move; the right value for a trainable one is a mistake there
    reset()
    put('w', right['w'])
    assert set(br.check_sunk(flat, before, ref.grads, 1e-6, index, frozen=('b',))) == {'w'}
    put('b', br.mistaken('frozen_written', base['b'], ref.grads['b']))
    with pytest.raises(AssertionError, match='frozen parameter'):
        br.check_sunk(flat, before, ref.grads, 1e-4, index, frozen=('b',))
    # one canary float
    reset()
    put('w', right['w']), put('b', right['b'])
    flat[index['canary']] = br.mistaken('neighbour_written', flat[index['canary']], flat[index['canary']])
    with pytest.raises(AssertionError, match='1 canary floats'):
        br.check_sunk(flat, before, ref.grads, 1e-4, index)
    assert set(br.MISTAKES) == {'overwrite', 'added_twice', 'frozen_written', 'neighbour_written',
                                'bias_from_weight_only_call_missing', 'unrequested_returned'}


# ---------------------------------------------------------------------------------- ops.dcn_multi behind the oracle
def _cpu_leaves(ref, req):
    return collections.OrderedDict((n, v.clone().requires_grad_(n in req)) for n, v in ref.leaves.items())


def test_dcn_multi_every_subset_behind_the_oracle(cpu_oracle_backend):
    """All 31 requests on the smallest DCNv2 case: what is asked for equals orc.deform_conv_backward, the rest is None."""
    case = br.DCN['xn']
    ref = br.reference(case)
    reqs = br.dcn_requests(case, everything=True)
    assert len(reqs) == 31
    for req in reqs:
        t = _cpu_leaves(ref, req)
        got = br.backward(br.dcn_outputs(case, t), ref.gos, t)
        br.check_request(got, ref.grads, req, ORACLE_TOL)


def test_pyramid_call_with_shared_and_detached_sources_behind_the_oracle(cpu_oracle_backend):
    case = br.DCN_PYR
    for unused in ((), (1,)):
        ref = br.reference(case, unused)
        for req in br.PYR_REQUESTS:
            t = _cpu_leaves(ref, req)
            outs = br.dcn_outputs(case, t)
            assert [tuple(o.shape[2:]) for o in outs] == [hw for _, hw in br.cfg_of(case)['levels']]
            br.check_request(br.backward(outs, ref.gos, t), ref.grads, req, ORACLE_TOL)


def test_fused_logits_form_behind_the_oracle(cpu_oracle_backend):
    """fused_om=True: ONE (B, 27, H, W) tensor of offsets | mask logits in, one gradient back -- [d offsets | d mask . m (1 - m)]
    of orc.deform_conv_backward."""
    from lsnet_amd import ops
    from oracle import oracle_py as orc
    case = br.DCN['xn']
    ref = br.reference(case)
    L = ref.leaves
    logits = torch.log(L['mask'] / (1 - L['mask']))
    m = torch.sigmoid(logits)
    g = orc.deform_conv_backward(L['x'], L['w'], L['off'], m, ref.gos[0], 1, 1, 1)
    want = dict(x=g['gx'].double(), om=torch.cat([g['goff'], g['gmask'] * m * (1 - m)], 1).double(), w=g['gw'].double(),
                b=g['gb'].double())
    for req in br.subsets(('x', 'om', 'w', 'b')):
        t = collections.OrderedDict(x=L['x'].clone(), om=torch.cat([L['off'], logits], 1), w=L['w'].clone(), b=L['b'].clone())
        for n, v in t.items():
            v.requires_grad_(n in req)
        outs = ops.dcn_multi([t['x']], [t['om']], None, t['w'], t['b'], 1, 1, 1, fused_om=True)
        br.check_request(br.backward(outs, ref.gos, t), want, req, ORACLE_TOL)


@pytest.mark.parametrize('state', ['all_sunk', 'weight_only', 'bias_frozen'])
def test_sinks_on_cpu_parameters_take_the_classic_path(state, cpu_oracle_backend):
    """Sinks registered on CPU parameters: the oracle backend has no `dcn_sinks_ok`, so _DCNFunction returns its
    gradients and AccumulateGrad ADDS them into the registered view; p.grad stays that view, nobody is told `done`."""
    from lsnet_amd.ops import grad_sink
    case = br.DCN['xn']
    ref, params, views, before, index = _arena_for(case, ('w', 'b'))
    done = []
    ps = {n: torch.nn.Parameter(p) for n, p in params.items()}
    sunk = ('w',) if state == 'weight_only' else ('w', 'b')
    for n in sunk:
        grad_sink.register(ps[n], views[n], on_done=lambda p: done.append(p))
        ps[n].grad = views[n]
        assert grad_sink.sink(ps[n]) is views[n]
    frozen = ('b',) if state == 'bias_frozen' else ()
    for n in frozen:
        ps[n].requires_grad_(False)
    t = collections.OrderedDict((n, v.clone()) for n, v in ref.leaves.items())
    t.update(ps)
    br.backward(br.dcn_outputs(case, t), ref.gos, t)
    for n in sunk:
        assert ps[n].grad is views[n] and ps[n].grad.data_ptr() == views[n].data_ptr()
    assert not done
    if state == 'weight_only':      # the bias has no sink: its gradient is a tensor of its own, the arena's view untouched
        assert br.rel_diff(ps['b'].grad.double(), ref.grads['b']) < ORACLE_TOL
        frozen = ('b',)
    br.check_sunk(index['flat'], before, ref.grads, ORACLE_TOL, index, frozen=frozen)
