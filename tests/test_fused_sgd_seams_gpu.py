"""lsn_clip_sgd_step (csrc/misc.hip: sgd_sqnorm_kernel, sgd_coef_kernel, sgd_step_kernel; planned by runner/fused_sgd.py) on
the storage it sees in training and at the sizes where it can go wrong: gradients as views of the reducer's packed
buckets with sentinels in every float it does not own, float4 / tail / chunk seams, more chunks than workgroups, tensor
tables of 1 .. 257 entries, several parameter groups, norms at the clipping threshold, zero, NaN and inf, and a plan that
adopts the momentum buffers of a run that is being resumed.  Layout, float64 reference, schedule and error measure:
tests/sgd_cases.py (run_case asserts, at every step: sentinels bit for bit, parameters / buffers / gradients within 2e-6 of
the largest operand against float64 and against torch's foreach and fused optimizers on the device, norm and coefficient
within 2e-6, untouched gradient bits when the coefficient is 1, and torch's bits in parameters and buffers on the
unclipped steps)."""
import ctypes

import pytest
import torch

from tests import sgd_cases as sc

pytestmark = pytest.mark.gpu

MAX_NORMS = [None, 3.0, 1e9]
DEV = torch.device('cuda:0')


def _plan(opt, clip):
    from lsnet_amd.runner.fused_sgd import ClipSGD
    return ClipSGD(opt, clip)


@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_seams_in_the_packed_layout(max_norm):
    """numel 1 .. 5 and 27, 4095 .. 4097, 8191 .. 8193 and three channels-last weights, back to back in the buckets"""
    recs = sc.run_case(_plan, DEV, sc.SEAMS, max_norm, seed=11)
    assert [r['coef'] < 1 for r in recs] == ([True] * 4 if max_norm == 3.0 else [False] * 4)


@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_more_chunks_than_workgroups(max_norm):
    """2138 chunks on 2048 workgroups: the chunk loop takes a second trip, on which workgroups 0, 1 and 78 .. 89 meet another
    tensor than on their first, and sgd_coef_kernel sums all 2048 partials"""
    chunks = sum((sc.numel(s) + 4095) // 4096 for s in sc.BIG)
    first = [sum((sc.numel(s) + 4095) // 4096 for s in sc.BIG[:i]) for i in range(len(sc.BIG))]
    assert 2048 < chunks < 4096 and first[1] < 2048 < first[2] and first[2] - 2048 < 2048
    sc.run_case(_plan, DEV, sc.BIG, max_norm, seed=12, bucket_mb=1.0)


@pytest.mark.parametrize('n', sc.TABLE_SIZES)
@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_tensor_tables_of_every_size(max_norm, n):
    """sgd_find over 1, 2, 3, 255, 256 and 257 entries (sizes 1 .. 6000, multi-chunk entries among them)"""
    sc.run_case(_plan, DEV, sc.table_shapes(n), max_norm, seed=13 + n, bucket_mb=0.004)


@pytest.mark.parametrize('groups', [sc.GROUPS3, sc.GROUPS8], ids=['three', 'eight'])
@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_parameter_groups(max_norm, groups):
    """own (lr, momentum, weight_decay) per group, one group without weight decay, neighbours in memory in different groups"""
    assert len({g[0] for g in groups}) == len({g[1] for g in groups}) == len({g[2] for g in groups}) == len(groups)
    sc.run_case(_plan, DEV, sc.MIXED, max_norm, groups=groups, seed=14)


def test_nine_groups_are_declined_before_any_state_exists():
    from lsnet_amd import _lib
    ps = [torch.nn.Parameter(torch.randn(8, device=DEV)) for _ in range(9)]
    for p in ps:
        p.grad = torch.randn_like(p)
    opt = torch.optim.SGD([dict(params=[p], lr=0.01 * (i + 1)) for i, p in enumerate(ps)], lr=0.1, momentum=0.9)
    plan = _plan(opt, dict(max_norm=3.0, norm_type=2))
    assert not plan.ok and len(opt.state) == 0
    eight = torch.optim.SGD([dict(params=[p], lr=0.01 * (i + 1)) for i, p in enumerate(ps[:8])], lr=0.1, momentum=0.9)
    assert _plan(eight, dict(max_norm=3.0, norm_type=2)).ok
    # the C entry itself: the arguments of a valid one-tensor call, but nine groups
    lib = _lib.load()
    p, g, b = torch.ones(8, device=DEV), torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    host = (_lib.SgdTensor * 1)()
    host[0].param, host[0].grad, host[0].momentum_buf, host[0].numel, host[0].first_chunk, host[0].group = \
        p.data_ptr(), g.data_ptr(), b.data_ptr(), 8, 0, 0
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    ws = torch.empty(int(lib.lsn_clip_sgd_workspace_bytes()), dtype=torch.uint8, device=DEV)
    stats = torch.zeros(2, device=DEV)
    groups = (_lib.SgdGroup * 9)()
    for q in groups:
        q.lr, q.momentum, q.weight_decay = 0.1, 0.9, 0.0

    def call(n_groups):
        return lib.lsn_clip_sgd_step(1, ctypes.c_void_p(table.data_ptr()), 1, n_groups, groups, ctypes.c_float(3.0),
                                     ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(9) != 0
    assert len(lib.lsn_last_error().decode()) > 0
    with pytest.raises(RuntimeError):
        _lib.check(call(9))
    torch.cuda.synchronize()
    assert torch.equal(p, torch.ones_like(p)) and torch.equal(b, torch.zeros_like(b))      # nothing was launched
    assert call(8) == 0
    torch.cuda.synchronize()
    assert not torch.equal(p, torch.ones_like(p))


@pytest.mark.parametrize('side', [-1, 1], ids=['just_below', 'just_above'])
@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_norm_at_the_clipping_threshold(max_norm, side):
    """step 1 clips at the float64 norm of its own gradients x (1 -+ 1e-3): the coefficient is below 1, respectively exactly 1
    (run_case asserts both against the reference; a changed max_norm rebuilds the plan, which adopts the buffers)"""
    recs = sc.run_case(_plan, DEV, sc.MIXED, max_norm, seed=15,
                       clip_at=lambda step, norm: norm * (1 + side * 1e-3) if step == 1 else max_norm)
    r = recs[1]
    if side < 0:
        assert r['coef'] < 1 and r['got_coef'] < 1 and abs(r['got_coef'] - (1 - 1e-3)) < 1e-5 and not r['grads_untouched']
    else:
        assert r['coef'] == 1 and r['got_coef'] == 1 and r['grads_untouched']


@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_all_zero_gradients(max_norm):
    """steps 1 and 2 have zero gradients: norm 0, coefficient 1, the gradients keep their bits, and the update is the
    weight-decay and momentum part alone"""
    recs = sc.run_case(_plan, DEV, sc.MIXED, max_norm, groups=sc.GROUPS3, seed=16,
                       edit=lambda step, gs: [torch.zeros_like(g) for g in gs] if step in (1, 2) else gs)
    for r in recs[1:3]:
        assert r['norm'] == 0 and r['coef'] == 1 and r['grads_untouched']
        if max_norm is not None:
            assert r['got_norm'] == 0 and r['got_coef'] == 1


def _poison(value):
    def edit(step, gs):
        if step != 1:
            return gs
        gs = list(gs)
        g = gs[4].clone()
        g[4096] = value                     # the one-float tail of the 4097-element tensor (group 1 of 3: no weight decay)
        gs[4] = g
        return gs
    return edit


@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_non_finite_gradient(max_norm, value):
    """One NaN or inf element in step 1.  With clipping a NaN makes norm, coefficient, every gradient and every parameter NaN
    (as clip_grad_norm_ does); an inf gives norm inf, coefficient 0, NaN in that element and a step from zero gradients
    everywhere else.  Without clipping the damage stays in that element.  run_case compares the NaN masks and the infs
    exactly and the finite rest by the bound."""
    recs = sc.run_case(_plan, DEV, sc.MIXED, max_norm, groups=sc.GROUPS3, seed=17, edit=_poison(value))
    total = sum(sc.numel(s) for s in sc.MIXED)
    r = recs[1]
    if max_norm is None:
        assert r['nonfinite_p'] == 1 and r['nonfinite_g'] == 1
    elif value != value:
        assert r['norm'] != r['norm'] and r['got_norm'] != r['got_norm'] and r['got_coef'] != r['got_coef']
        assert r['nonfinite_p'] == total and r['nonfinite_g'] == total
    else:
        assert r['got_norm'] == float('inf') and r['got_coef'] == 0.0
        assert r['nonfinite_p'] == 1 and r['nonfinite_g'] == 1
    assert recs[0]['nonfinite_p'] == 0


@pytest.mark.parametrize('max_norm', MAX_NORMS)
def test_resumed_training(max_norm):
    """Two steps of clip_grad_norm_ + optimizer.step() first; the plan built then adopts the buffers torch made (the same
    tensor objects, not zeroed: run_case asserts it) and goes on equal to torch carrying on.  Before step 4 the optimizer's
    state is reloaded from a deep copy of its state_dict: still_valid() is False, a rebuilt plan is ok and goes on equal."""
    recs = sc.run_case(_plan, DEV, sc.MIXED, max_norm, groups=sc.GROUPS3, seed=18, steps=6, torch_first=2, reload_before=4)
    assert len(recs) == 6
