"""The case tables of tests/conv_geometry_cases.py, checked on the CPU without the library.

Two properties of every case.  It lies inside the limits the library states (include/lsnet_hip.h, csrc/conv.hip conv_check and
bwd_plan: a non-empty output, at most 64 taps, at most 64 residue classes).  And it DISCRIMINATES: the fp64 evaluation of a
plausible mistake of its group -- taps transposed, padding off by one, the stride phase shifted by one input pixel, images
swapped, the last output channel dropped or duplicated -- differs from the fp64 reference by at least 1e-3 of the reference's
range in the output and in both gradients, 20 times the loosest tolerance of the device test.  A case on which its mistake
is invisible (a symmetric input, a map the padding swallows) would pass on a wrong kernel: it gets another shape or seed,
never a lower threshold."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_geometry_cases as cg

DISCRIMINATES = 1e-3
IDS = [cg.case_id(c) for c in cg.ALL]


def test_tables_cover_what_they_claim():
    assert len(set(IDS)) == len(IDS) and len({c.seed for c in cg.ALL}) == len(cg.ALL)
    for group in range(1, 7):       # the four forward tiles, both chunk counts, and the wide row in every tiled group
        cs = [c for c in cg.GENERIC if c.group == group]
        assert {c.Co for c in cs} >= set(cg.TILE_CO) and {c.C for c in cs} >= set(cg.TILE_C), group
        assert any(c.C == 64 and c.Co == 256 and c.kh * c.kw >= 9 and c.B * cg.out_shape(c)[2] * cg.out_shape(c)[3] >= 4096 for c in cs)
    for geom in {(c.kh, c.kw, c.s, c.p, c.d, c.H, c.W) for c in cg.GENERIC if c.group <= 6 and c.C in cg.TILE_C}:
        assert {c.Co for c in cg.GENERIC if (c.kh, c.kw, c.s, c.p, c.d, c.H, c.W) == geom} >= set(cg.TILE_CO), geom
    px = lambda c: c.B * cg.out_shape(c)[2] * cg.out_shape(c)[3]
    # two pixel tiles with a ragged tail wherever the group is not about tiny maps (128-pixel tiles for Co <= 64, 64 beyond)
    for c in cg.GENERIC:
        if c.group in (1, 2, 3, 4, 7):
            assert px(c) > 128 and px(c) % 128 and c.B * c.H * c.W > 128, cg.case_id(c)
    # a ReLU output whose size is no multiple of 4 (the `go * (out > 0)` branch of _ConvFn.backward) and one that is
    assert any(px(c) * c.Co % 4 for c in cg.GENERIC) and any(px(c) * c.Co % 4 == 0 for c in cg.GENERIC)
    # batches: a 128-pixel tile holds more than one image
    assert all(cg.out_shape(c)[2] * cg.out_shape(c)[3] < 64 for c in cg.BATCH if c.Co != 256 or c.C != 64)
    assert {c.B for c in cg.BATCH} >= {3, 5, 8}
    # padding beyond (k - 1) dil: bwd_plan's forward kernel gets a negative pad
    assert any(c.p > (c.kh - 1) * c.d for c in cg.PAD) and any(c.p == 0 and c.kh == 3 for c in cg.PAD)
    rows = [c for c, _ in cg.ROW_MERGED]
    assert {c.C for c in rows} == {1, 3, 4, 5, 7} and {c.s for c in rows} == {1, 2, 3} and {c.p for c in rows} == {0, 1, 3, 4}
    assert {c.Co for c in rows} == {8, 27, 64, 96} and {(c.kh, c.kw) for c in rows} == {(3, 3), (5, 5), (7, 7), (3, 5), (1, 3)}
    assert {(r, c.bias) for c, r in cg.ROW_MERGED} == {(False, False), (False, True), (True, False), (True, True)}
    assert all(c.C < 8 and c.kw > 1 and c.d == 1 for c in rows) and len(rows) >= 20


@pytest.mark.parametrize('c', cg.ALL, ids=IDS)
def test_case_is_inside_the_stated_limits(c):
    _, _, Ho, Wo = cg.out_shape(c)
    assert Ho > 0 and Wo > 0 and c.kh * c.kw <= 64 and c.s * c.s <= 64
    assert min(c.B, c.C, c.Co, c.H, c.W, c.s, c.d) > 0 and c.p >= 0


@pytest.mark.parametrize('c', cg.ALL, ids=IDS)
def test_case_discriminates(c):
    x, w, b, go = cg.inputs(c)
    y, gx, gw, _ = cg.reference(c)[4]
    # the window form the mistakes are written in is the convolution when nothing is wrong
    same = cg._windows(x.double(), w.double(), None if b is None else b.double(), c, c.p, c.p)
    assert cg.rel_diff(same, y) < 1e-12
    for kind in cg.MISTAKES[c.group]:
        if kind == 'last_channel_duplicated' and c.Co == 1:
            continue
        my, mgx, mgw = cg.mistaken_ref(kind, c)
        assert my.shape == y.shape
        for name, m, r in (('y', my, y), ('gx', mgx, gx), ('gw', mgw, gw)):
            assert cg.rel_diff(m, r) >= DISCRIMINATES, (kind, name, cg.rel_diff(m, r))


def test_gated_reference_leaves_no_gate_near_zero():
    """relu=True: wherever the fp64 pre-activation is within 1e-3 of the range of zero the output gradient is zero, so the
    gradients do not depend on which side of zero an fp32 kernel puts it; the margin removes a small share of the elements."""
    c = cg.RECT[0]
    x, w, b, go, (y, gx, gw, gb) = cg.reference(c, relu=True)
    pre = F.conv2d(x.double(), w.double(), None if b is None else b.double(), c.s, c.p, c.d)
    near = pre.abs() <= cg.GATE_MARGIN * pre.abs().max()
    assert near.any() and float(near.double().mean()) < 0.01
    assert (go[near] == 0).all() and (go[~near] != 0).all()
    assert torch.equal(y, F.relu(pre))
    flipped = torch.where(near, -pre, pre)          # every doubtful gate on the other side: the same gradients
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = F.conv2d(xr, wr, None if b is None else b.double(), c.s, c.p, c.d)
    g2 = torch.autograd.grad(yr, [xr, wr], go.double() * (flipped > 0))
    assert torch.equal(g2[0], gx) and torch.equal(g2[1], gw)
