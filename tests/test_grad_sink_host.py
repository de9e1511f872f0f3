"""ops/grad_sink.py `claim`: the one decision "does this backward call ADD into the parameters' gradient sinks or return
fresh tensors", on CPU tensors and without the library.  The expected answers are the rules of the operators, written
out per parameter set:

  (w, bias), bias optional   conv2d, conv2d_multi, the deformable family: w wanted and sunk; bias unwanted or sunk;
                             the sink has w's strides
  (gamma, beta)              bn_act, GroupNorm: both wanted and sunk
  (w, gamma, beta)           conv_bn_act (wgrad_bn, and deferred: wgrad_bn_jobs): all three wanted and sunk; strides

A sink is live when it is registered and `p.grad is` it; all-or-nothing per call."""
import collections
import itertools
import types

import pytest
import torch

from lsnet_amd.ops import grad_sink

_CL = torch.channels_last
STATES = ('sunk', 'none', 'replaced')

# name -> (parameter names, optional positions, accumulate?(wanted names, names with a live sink))
SETS = {
    'w_bias': (('w', 'bias'), (1,),
               lambda want, live: 'w' in want and 'w' in live and ('bias' not in want or 'bias' in live)),
    'gamma_beta': (('gamma', 'beta'), (),
                   lambda want, live: want == {'gamma', 'beta'} and live == {'gamma', 'beta'}),
    'w_gamma_beta': (('w', 'gamma', 'beta'), (),
                     lambda want, live: want == {'w', 'gamma', 'beta'} and live == {'w', 'gamma', 'beta'}),
}


def _param(name):
    if name == 'w':
        return torch.nn.Parameter(torch.randn(6, 4, 3, 3).contiguous(memory_format=_CL))
    return torch.nn.Parameter(torch.randn(6))


def _setup(names, states, view_of=torch.zeros_like):
    """parameters in the given sink states -> (params, registered views, Counter of on_done calls by name)"""
    params = collections.OrderedDict((n, _param(n)) for n in names)
    views, done = {}, collections.Counter()
    for (n, p), state in zip(params.items(), states):
        if state == 'none':
            continue
        views[n] = view_of(p)
        grad_sink.register(p, views[n], on_done=lambda p, n=n: done.update([n]))
        p.grad = views[n] if state == 'sunk' else torch.zeros_like(p)      # 'replaced': registered, but p.grad is another tensor
    return params, views, done


def _subsets(names):
    return [set(s) for k in range(1, len(names) + 1) for s in itertools.combinations(names, k)]


@pytest.mark.parametrize('which', list(SETS))
def test_claim_over_wanted_patterns_and_sink_states(which):
    names, optional, rule = SETS[which]
    seen = collections.Counter()
    for want in _subsets(names):
        for states in itertools.product(STATES, repeat=len(names)):
            params, views, done = _setup(names, states)
            live = {n for n, s in zip(names, states) if s == 'sunk'}
            assert all(v.stride() == params[n].stride() for n, v in views.items())
            c = grad_sink.claim([(params[n], n in want) for n in names], optional=optional)
            expect = rule(want, live)
            seen[expect] += 1
            what = (which, sorted(want), states)
            assert c.accumulate == (1 if expect else 0), what
            fresh = [torch.empty(1) for _ in names]
            res = c.results(fresh)
            assert len(c.sinks) == len(res) == len(names), what
            for i, n in enumerate(names):
                if expect:      # the registered view itself where wanted; nothing comes back; its owner is told once
                    assert c.sinks[i] is (views[n] if n in want else None), (what, n)
                    assert res[i] is None, (what, n)
                    assert done[n] == (1 if n in want else 0), (what, n, done)
                else:           # no buffer of the claim's; the site's own tensor where wanted; nobody is told
                    assert c.sinks[i] is None, (what, n)
                    assert res[i] is (fresh[i] if n in want else None), (what, n)
                    assert done[n] == 0, (what, n, done)
    assert seen[True] and seen[False], seen
    # (w, bias): w alone onto its sink whatever the bias has (3 states), both onto theirs (1); the norms: one combination
    assert seen[True] == (4 if which == 'w_bias' else 1), seen


def test_a_missing_bias_is_an_unwanted_one():
    """conv2d without a bias hands (None, False); a caller that says True for a None parameter gets the same"""
    for want_b in (False, True):
        params, views, done = _setup(('w',), ('sunk',))
        c = grad_sink.claim([(params['w'], True), (None, want_b)], optional=(1,))
        assert c.accumulate == 1 and c.sinks[0] is views['w'] and c.sinks[1] is None
        assert c.results((torch.empty(1), None)) == (None, None) and done == collections.Counter(w=1)
    params, views, done = _setup(('w',), ('none',))
    c = grad_sink.claim([(params['w'], True), (None, False)], optional=(1,))
    gw = torch.empty(1)
    res = c.results((gw, None))
    assert c.accumulate == 0 and res[0] is gw and res[1] is None and not done


@pytest.mark.parametrize('which', ['w_bias', 'w_gamma_beta'])
def test_a_sink_with_other_strides_than_its_channels_last_weight_is_not_used(which):
    """every parameter wanted and sunk, but w's sink is a contiguous tensor under a channels-last weight: the classic path"""
    names, optional, _ = SETS[which]
    params, views, done = _setup(names, ('sunk',) * len(names),
                                 view_of=lambda p: torch.zeros(p.shape) if p.dim() == 4 else torch.zeros_like(p))
    assert views['w'].stride() != params['w'].stride() and grad_sink.sink(params['w']) is views['w']
    c = grad_sink.claim([(params[n], True) for n in names], optional=optional)
    fresh = [torch.empty(1) for _ in names]
    res = c.results(fresh)
    assert c.accumulate == 0 and all(s is None for s in c.sinks)
    assert all(r is f for r, f in zip(res, fresh)) and not done


def test_an_operator_without_sink_support_claims_nothing():
    """`allowed=False` (GroupNorm behind a backend without `supports_grad_sinks`, a deformable call the backend declines)"""
    params, views, done = _setup(('gamma', 'beta'), ('sunk', 'sunk'))
    c = grad_sink.claim([(params['gamma'], True), (params['beta'], True)], allowed=False)
    fresh = [torch.empty(1), torch.empty(1)]
    res = c.results(fresh)
    assert c.accumulate == 0 and c.sinks == [None, None] and res[0] is fresh[0] and res[1] is fresh[1] and not done


class _FakeParam:
    """what a claim reads of a parameter (its strides, .grad, the registration), with `is_cuda` free to choose"""

    def __init__(self, like, is_cuda):
        self._like, self.is_cuda, self.grad = like, is_cuda, None

    def stride(self):
        return self._like.stride()


@pytest.mark.parametrize('is_cuda', [False, True])
def test_wgrad_bn_deferrable_is_the_claim_over_all_three(is_cuda):
    """wgrad_bn_deferrable(w, bn) == "a claim over (w, gamma, beta), all wanted, accumulates" and w on the device: every
    combination of sink states, on stand-ins that say where they live (no device is touched); and on real CPU parameters,
    where the claim accumulates and the answer is still no."""
    from lsnet_amd.ops.conv import wgrad_bn_deferrable
    names = ('w', 'gamma', 'beta')
    for states in itertools.product(STATES, repeat=3):
        ps = {}
        for n, state in zip(names, states):
            like = _param(n)
            ps[n] = _FakeParam(like, is_cuda)
            if state != 'none':
                view = torch.zeros_like(like)
                grad_sink.register(ps[n], view)
                ps[n].grad = view if state == 'sunk' else torch.zeros_like(like)
        bn = types.SimpleNamespace(weight=ps['gamma'], bias=ps['beta'])
        got = wgrad_bn_deferrable(ps['w'], bn)
        assert got is (is_cuda and states == ('sunk', 'sunk', 'sunk')), (states, got)
        assert got == bool(grad_sink.claim([(ps[n], True) for n in names]).accumulate and is_cuda), states
    if not is_cuda:
        params, _, done = _setup(names, ('sunk',) * 3)
        bn = types.SimpleNamespace(weight=params['gamma'], bias=params['beta'])
        assert grad_sink.claim([(params[n], True) for n in names]).accumulate == 1
        assert wgrad_bn_deferrable(params['w'], bn) is False and not done
