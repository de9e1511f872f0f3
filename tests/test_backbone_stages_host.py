"""The stage cases of tests/backbone_stage_cases.py on the host: the package's own host path (the blocks' `_body` in fp32 on
CPU tensors, deformable convs through the oracle backend -- the code tests/test_live_reference.py pins to the reference) against
the float64 restatement, under the bound the device is held to; the two conditions that make a hard maximum bound on gradients
legitimate; no parameter without a gradient; and four deliberately wrong restatements that the bound must notice."""
import copy

import pytest
import torch

from tests import backbone_stage_cases as C


@pytest.mark.parametrize('name', list(C.CASES))
def test_host_path_equals_fp64(name, cpu_oracle_backend):
    ref = C.reference(name)
    layer = C.as_trained(copy.deepcopy(ref.layer))
    x = ref.x.clone().requires_grad_()
    y = x
    for blk in layer:
        y = blk._body(y)
    y.backward(ref.go)
    got = {'out': y, 'x': x.grad}
    for k, p in layer.named_parameters():
        assert p.grad is not None, k
        got[k] = p.grad
    assert set(got) == set(ref.f64)
    rows = C.compare(ref, got)
    C.report(f'{name} host', rows)
    assert not C.failures(rows), C.failures(rows)


@pytest.mark.parametrize('name', list(C.CASES))
def test_conditions_hold(name):
    """Kink and lattice clearance on the built case, from a float64 run of its own; every block's ReLUs and every deformable
    conv's coordinates are among the events."""
    ref = C.reference(name)
    trace = C.Trace()
    with torch.no_grad():
        C.stage_fp64(copy.deepcopy(ref.layer).double(), ref.x.double(), trace)
    relus = [e for e in trace.events if e[0] == 'relu']
    coords = [e for e in trace.events if e[0] == 'coord']
    per_block = {'Bottleneck': 3, 'BasicBlock': 2, 'Bottle2neck': 5}[C.CASES[name][1]]
    assert len(relus) == per_block * len(ref.layer)
    dcns = sum(hasattr(m, 'conv_offset') for m in ref.layer.modules())
    assert len(coords) == dcns and (dcns > 0) == (name in C.DCN_CASES)
    for _, what, t, _ in relus:
        assert float(t.abs().min()) >= C.DELTA * float(t.abs().max()), what
    for _, what, c, _ in coords:
        assert float((c - c.round()).abs().min()) >= C.LATTICE, what
        # the offsets do what the golden backbones never do: they differ per pixel, and some samples leave the map
        m = ref.layer.get_submodule(what)
        off = c - C.sampling_coords(torch.zeros_like(c), C._first(m.stride), C._first(m.padding), C._first(m.dilation), 3, 3)
        assert float(off.std(dim=(0, 2, 3)).min()) > 0.1, what
    if coords:
        h, w = (C.H, C.W)
        rows = torch.cat([c[:, 0::2].flatten() for _, _, c, _ in coords])
        cols = torch.cat([c[:, 1::2].flatten() for _, _, c, _ in coords])
        assert bool((rows < -1).any() or (rows > h).any() or (cols < -1).any() or (cols > w).any())
    assert not C.violations(trace)


@pytest.mark.parametrize('name', list(C.CASES))
def test_no_dead_parameters(name):
    ref = C.reference(name)
    assert set(ref.f64) == {'out', 'x'} | {k for k, _ in ref.layer.named_parameters()}
    for k, g in ref.f64.items():
        assert float(g.abs().max()) > 0, k
    last = ref.layer[-1]
    norm = last.norm3 if hasattr(last, 'norm3_name') else last.norm2
    key = f'{len(ref.layer) - 1}.{last.norm3_name if hasattr(last, "norm3_name") else last.norm2_name}.weight'
    assert float(norm.weight.detach()[:4].abs().max()) == 0 and float(ref.f64[key][:8].abs().min()) > 0


@pytest.mark.parametrize('wrong', list(C.WRONG_STATEMENTS))
def test_bound_notices_wrong_statements(wrong):
    ref = C.reference(C.WRONG_STATEMENTS[wrong])
    got = C.evaluate(copy.deepcopy(ref.layer).double(), ref.x.double(), ref.go.double(), wrong=wrong)
    rows = C.compare(ref, got)
    worst = max(rows, key=lambda r: r[1] / r[3])
    print(f'STAGE {ref.name} {wrong}: {worst[0]} leaves by {worst[1]:.3e} = {worst[1] / worst[3]:.0f} x its bound')
    assert worst[1] >= 100 * worst[3], worst
