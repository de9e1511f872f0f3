"""The CPU oracle at kernel sizes other than 3 x 3 (tests/dcn_kernel_size_cases.py): forward and all five gradients against the
independent torch restatement (tests/torch_dcn_ref.py) evaluated in float64, at the bound tests/test_oracle.py holds the 3 x 3
cases to.  The GPU tests of these cases compare against the oracle, so this is what makes it a reference there.  No GPU."""
import pytest
import torch

from tests import dcn_kernel_size_cases as ks
from tests.torch_dcn_ref import torch_dcn

BOUND = 1e-5   # tests/test_oracle.py test_forward_backward_against_torch_restatement


def _rel(a, b):
    return (a.double() - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


@pytest.mark.parametrize('name', ks.NAMES)
def test_oracle_against_float64_restatement(name):
    (x, w, b, off, mask, go, cfg), out, grads = ks.reference(name)
    leaves = [t.double().requires_grad_() if t is not None else None for t in (x, off, mask, w, b)]
    xd, od, md, wd, bd = leaves
    ref = torch_dcn(xd, od, md, wd, bd, cfg['stride'], cfg['pad'], cfg['dil'], cfg['groups'], cfg['dg'], cfg['sh'], cfg['sw'])
    assert ref.dtype == torch.float64 and tuple(ref.shape[2:]) == cfg['out_hw']
    names = ['gx', 'goff'] + (['gmask'] if mask is not None else []) + ['gw'] + (['gb'] if b is not None else [])
    grefs = torch.autograd.grad(ref, [t for t in leaves if t is not None], go.double())
    errs = {'out': _rel(out, ref.detach())}
    for n, g in zip(names, grefs):
        errs[n] = _rel(grads[n], g)
    print(name, {k: f'{v:.1e}' for k, v in errs.items()})
    assert all(e < BOUND for e in errs.values()), errs
    if b is None:   # (the oracle always returns the bias gradient: the sum of grad_output over pixels)
        assert _rel(grads['gb'], go.double().sum((0, 2, 3))) < BOUND


def test_case_table_is_within_its_own_limits():
    """Maps at or below 13 x 21, reduction depth at or below 4608, the KD every row of the table states."""
    for c in ks.CASES:
        kh, kw = c['k']
        assert max(c['hw'][0], c.get('dst', (0, 0))[0]) <= 13 and max(c['hw'][1], c.get('dst', (0, 0))[1]) <= 21, c['name']
        assert c['C'] // c.get('groups', 1) * kh * kw <= 4608, c['name']
    want = dict(k1_one_chunk=1, k5_pyr=25, k5_dg2=50, k7_narrow=49, k7_dil2=49, k8_bound=64, k4_dg4_bound=64, k5_dg3_over=75)
    assert {n: ks.kd(ks.case(n)) for n in want} == want
    assert set(ks.ROUTES) == set(ks.NAMES) - {'k5_dg3_over'}
    assert {k[0] for k in ks.EXPECTED_REFUSALS} <= set(ks.NAMES)
    # the bound of include/lsnet_hip.h from the formula it quotes: the fp32 scatter's 64-wide slab, 8 KiB + 2816 B per tap
    assert ks.kd_every_route() == (160 * 1024 - 8192) // 2816 == 55
    # every refusal of the table is above the bound
    assert all(ks.kd(ks.case(n)) > ks.kd_every_route() for n, _, _ in ks.EXPECTED_REFUSALS)
