"""runner/fused_sgd.py without a GPU: the plan declines everything the library's clip + SGD step does not do (the hook then
keeps clip_grad_norm_ + optimizer.step(), mmcv/runner/hooks/optimizer.py:8-28), and the host-side fall-backs of the round-4
glue (core/assigners.py: topk_columns, ops/dcn.py: offset_scale_chain) are the torch statements they replace."""
import pytest
import torch

from lsnet_amd.core.assigners import topk_columns
from lsnet_amd.ops.dcn import offset_scale_chain
from lsnet_amd.runner.fused_sgd import ClipSGD
from tests import sgd_cases as sc


def _params():
    ps = [torch.nn.Parameter(torch.randn(8, 4, 3, 3)), torch.nn.Parameter(torch.randn(8))]
    for p in ps:
        p.grad = torch.randn_like(p)
    return ps


def test_plan_declines_what_the_library_does_not_do():
    clip = dict(max_norm=35, norm_type=2)
    ps = _params()
    assert not ClipSGD(torch.optim.SGD(ps, lr=0.1, momentum=0.9), clip).ok                     # host tensors
    assert not ClipSGD(torch.optim.Adam(ps, lr=0.1), clip).ok                                  # not SGD
    assert not ClipSGD(torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True), clip).ok
    assert not ClipSGD(torch.optim.SGD(ps, lr=0.1, momentum=0.0), clip).ok                     # no momentum buffer to keep
    assert not ClipSGD(torch.optim.SGD(ps, lr=0.1, momentum=0.9), dict(max_norm=35, norm_type=1)).ok
    assert not ClipSGD(torch.optim.SGD(ps, lr=0.1, momentum=0.9), dict(max_norm=0.0, norm_type=2)).ok


@pytest.mark.parametrize('max_norm', [None, 3.0, 1e9])
def test_reference_step_is_torch_in_float64(max_norm):
    """What the GPU cases compare against (tests/sgd_cases.py: reference_step) against clip_grad_norm_ + torch.optim.SGD in
    float64 on the CPU: three parameter groups (one without weight decay) dealt round-robin, four steps with the GPU cases'
    schedule, to 1e-12."""
    shapes = sc.MIXED
    p0, grads = sc.draw(shapes, 21)
    group_of = [i % 3 for i in range(len(shapes))]
    ps = [torch.nn.Parameter(t.double()) for t in p0]
    opt = sc.make_sgd(ps, sc.GROUPS3)
    P, B = [t.double() for t in p0], [None] * len(shapes)
    clipped = []
    for step in range(sc.STEPS):
        g64 = [g.double() for g in grads[step]]
        for p, g in zip(ps, g64):
            p.grad = g.clone()
        sc.set_lr(opt, sc.GROUPS3, step)
        tnorm = None if max_norm is None else torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2)
        opt.step()
        P, B, G, norm, coef = sc.reference_step(P, g64, B, [(lr * (step + 1), m, wd) for lr, m, wd in sc.GROUPS3], group_of, max_norm)
        clipped.append(float(coef) < 1)
        if tnorm is not None:
            assert abs(float(norm) - float(tnorm)) <= 1e-12 * float(tnorm)
        for p, a, b, g in zip(ps, P, B, G):
            assert float((p.detach() - a).abs().max()) <= 1e-12
            assert float((opt.state[p]['momentum_buffer'] - b).abs().max()) <= 1e-12
            assert float((p.grad - g).abs().max()) <= 1e-12
    assert clipped == {None: [False] * 4, 3.0: [True] * 4, 1e9: [False] * 4}[max_norm]


def test_reference_step_on_non_finite_gradients_is_torch():
    """inf with clipping: coefficient 0, that element NaN, the others stepped from a zero gradient; NaN with clipping:
    everything NaN; at weight_decay 0 an inf parameter stays inf (torch adds no 0 * p)."""
    for bad, wd in ((float('inf'), 0.0), (float('nan'), 1e-4), (float('inf'), 1e-4)):
        for max_norm in (None, 3.0):
            p0 = [torch.randn(5, dtype=torch.float64), torch.randn(3, dtype=torch.float64)]
            g0 = [torch.randn(5, dtype=torch.float64), torch.randn(3, dtype=torch.float64)]
            g0[0][2] = bad
            ps = [torch.nn.Parameter(t.clone()) for t in p0]
            opt = torch.optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=wd)
            P, B = p0, [None, None]
            for _ in range(2):
                for p, g in zip(ps, g0):
                    p.grad = g.clone()
                if max_norm is not None:
                    torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2)
                opt.step()
                P, B, G, norm, coef = sc.reference_step(P, g0, B, [(0.1, 0.9, wd)], [0, 0], max_norm)
                for p, a, b in zip(ps, P, B):
                    assert torch.allclose(p.detach(), a, rtol=0, atol=1e-12, equal_nan=True)
                    assert torch.allclose(opt.state[p]['momentum_buffer'], b, rtol=0, atol=1e-12, equal_nan=True)
            if max_norm is not None and bad != bad:
                assert all(bool(t.isnan().all()) for t in P)
            if max_norm is None:
                assert sum(int((~t.isfinite()).sum()) for t in P) == 1


def test_layout_is_the_training_layout_and_its_sentinels_are_watched():
    """tests/sgd_cases.py: Layout on the host -- gradients are views of a several-bucket arena of the reducer itself, slots are
    rounded to 4 floats, every view starts on 16 bytes, and a changed pad float of any of the three flat tensors is seen."""
    lay = sc.Layout(sc.SEAMS, torch.device('cpu'))
    assert lay.n_buckets >= 3 and lay.reducer.arena is not None
    arena = lay.reducer.arena
    for p, b, s in zip(lay.params, lay.bufs, sc.SEAMS):
        g = p.grad
        assert g.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()      # p.grad IS a bucket view
        assert g.shape == p.shape == b.shape and g.stride() == p.stride() == b.stride()
        assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        assert p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)
    # 1, 2, 3, 5, 27, 4095, 4097, 8191, 8193 and 5*3 leave 3+2+1+3+1+1+3+1+3+1 = 19 pad floats in a slot
    slots = sum((sc.numel(s) + 3) // 4 * 4 - sc.numel(s) for s in sc.SEAMS)
    assert slots == 19 and lay.pad_floats() >= 3 * 19 + 4 * sc.GUARD
    assert lay.damaged() == []
    for p in lay.params:
        p.data.normal_(), p.grad.normal_()
    for b in lay.bufs:
        b.zero_()
    assert lay.damaged() == []                       # writing the views themselves touches no pad
    lay.grads[0].as_strided((2,), (1,))[1] = 0.0     # the float behind the one-element gradient
    assert lay.damaged() == ['grad']
    lay.params[5].data.as_strided((28,), (1,))[27] = 0.0     # the float behind the 27-element parameter
    lay.flat_b[-1] = 1.0                             # the guard band
    assert lay.damaged() == ['param', 'momentum', 'grad']
    # a load of a pad cannot go unnoticed either: its square is not a finite fp32 number
    assert float(torch.tensor(sc.SENTINEL, dtype=torch.float32) ** 2) == float('inf')


def test_topk_columns_on_the_host_is_torch_topk():
    g = torch.Generator().manual_seed(0)
    x = torch.randperm(400 * 5, generator=g).float().reshape(400, 5)
    v, i = topk_columns(x, 3)
    vr, ir = x.topk(3, dim=0, largest=False)
    assert torch.equal(v, vr) and torch.equal(i, ir)
    segs = [(0, 250), (250, 100), (350, 50)]
    v, i = topk_columns(x, 4, segs, largest=True)
    for s, (start, n) in enumerate(segs):
        vr, ir = x[start:start + n].topk(4, dim=0, largest=True)
        assert torch.equal(v[4 * s:4 * s + 4], vr) and torch.equal(i[4 * s:4 * s + 4], ir + start)


def test_offset_scale_chain_on_the_host_is_the_multiplication_sequence():
    g = torch.Generator().manual_seed(1)
    offs = [torch.randn(2, 18, 5, 7, generator=g, requires_grad=True), torch.randn(2, 18, 3, 4, generator=g, requires_grad=True)]
    mults = [((0.5, 0.52), (2.0, 25 / 13), (0.28, 11 / 42)), ((1.0, 1.0), (13 / 7, 21 / 11), (7 / 13, 0.5))]
    first, second = offset_scale_chain(offs, mults, copies=2)
    assert first is second or all(a is b for ta, tb in zip(first, second) for a, b in zip(ta, tb))   # host: the same tensors
    for off, m, trio in zip(offs, mults, first):
        cur = off
        for (sh, sw), t in zip(m, trio):
            cur = cur * off.new_tensor([sh, sw]).repeat(9).view(1, -1, 1, 1)
            assert torch.equal(t, cur)
    sum(t.sum() for trio in first for t in trio).backward()
    assert all(o.grad is not None for o in offs)
