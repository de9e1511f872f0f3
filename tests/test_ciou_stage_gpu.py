"""The whole-stage polygon / keypoint cross-IOU kernels (csrc/loss.hip: lsn_cross_iou_stage_forward / _backward, through
ops.cross_iou.cross_iou_stage_rows) on the device against the float64 statement of LSHead.loss_levels + cross_iou_loss at
the inputs of tests/loss_stage_cases.py; the seams of the 64-row tile, odd storage, mismatched side tensors, and the route
LSHead.loss_levels takes for the segm and pose tasks.

Rule (tests.cpv_cases.judge; per row for the gradient, loss_edge_cases.judge_rows): the native arm's error against float64 may
be at most twice that of the same statements in fp32 torch on the device, or 1e-6 where that is larger.  No row is masked."""
import pytest
import torch

from tests import loss_edge_cases as lec
from tests import loss_stage_cases as lsc
from tests.cpv_cases import judge

pytestmark = pytest.mark.gpu

R = 64          # rows per tile of the kernel


def _dev():
    return torch.device('cuda:0')


def _on(case, dev):
    return {k: v.to(dev) for k, v in case.items()}


def _native(kind, c, alpha, sub, n=None, **over):
    """cross_iou_stage_rows on the first n rows of a case that lies on the device -> (rows, d sum(rows * up) / d raw);
    `over`: tensors that replace the case's"""
    from lsnet_amd.ops import cross_iou as fused
    n = c['raw'].shape[0] if n is None else n
    a = {k: v[:n].clone() for k, v in c.items()}
    a.update(over)
    p = a['raw'].requires_grad_()
    rows = fused.cross_iou_stage_rows(kind, p, a['gt_pts'], a['anchor3'], a['box'], a['vs'], a['weight'], lec.BASE_SCALE, alpha,
                                      1e-6, sub)
    g, = torch.autograd.grad(rows, p, a['up'])
    return rows.detach(), g


_FULL = {}


def _full(kind, nv, sub, alpha=0.25):
    """the plain call on the 1,500-row case, once per module"""
    key = (kind, nv, sub, alpha)
    if key not in _FULL:
        _FULL[key] = _native(kind, _on(lsc.shared_case(kind, nv, sub), _dev()), alpha, sub)
    return _FULL[key]


@pytest.mark.parametrize('alpha', lsc.ALPHAS)
@pytest.mark.parametrize('kind,nv,sub', lsc.CASES)
def test_stage_rows_against_the_head_formulation(kind, nv, sub, alpha):
    case = lsc.shared_case(kind, nv, sub)
    what = f'stage {kind} nv {nv} sub {sub} alpha {alpha}'
    ref, gref = lsc.reference(kind, nv, sub, alpha)
    assert torch.isfinite(ref).all() and torch.isfinite(gref).all(), what          # every row, none masked out
    assert lec.decisions_agree(case['raw'], *lsc.stage_targets(case, torch.float32), alpha), what
    t32, g32 = lsc.stage_statement(kind, case, alpha, torch.float32, _dev(), sub)
    rows, g = _full(kind, nv, sub, alpha)
    assert rows.shape == (lsc.N_ROWS,) and g.shape == case['raw'].shape
    judge(rows, t32, ref, what + ' loss')
    lec.judge_rows(g, g32, gref, what + ' grad')
    dead = (case['weight'] == 0).to(_dev())
    assert dead.sum() >= 500 and not rows[dead].any() and not g[dead].any(), what


@pytest.mark.parametrize('kind,nv,sub', [('polygon', 36, 9), ('polygon', 9, 9), ('keypoint', 17, 9), ('keypoint', 1, 9)])
def test_tile_seams_give_the_bits_of_the_long_call(kind, nv, sub):
    """n = 0, 1, one row short of a tile, a tile, a tile and a row, four tiles and a row: the first n rows of the 1,500-row
    call, bit for bit.  (The launch has one workgroup per tile and no cap on its grid.)"""
    c = _on(lsc.shared_case(kind, nv, sub), _dev())
    full, gfull = _full(kind, nv, sub)
    for n in (0, 1, R - 1, R, R + 1, 257):
        rows, g = _native(kind, c, 0.25, sub, n)
        assert rows.shape == (n,) and g.shape == (n, 4 * (nv + 1))
        assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n]), n


@pytest.mark.parametrize('kind,nv,sub', [('polygon', 36, 9), ('keypoint', 17, 9)])
def test_odd_storage_equals_the_plain_call(kind, nv, sub):
    """a column slice of a wider tensor, rows at a 4-byte offset of their buffer (contiguous, but not 16-byte aligned: they
    are copied), an expanded upstream gradient, int64 visibilities: the same bits as the plain call"""
    dev, n, m = _dev(), 257, 4 * (nv + 1)
    c = _on(lsc.shared_case(kind, nv, sub), dev)
    full, gfull = _full(kind, nv, sub)
    wide = torch.zeros(n, m + 12, device=dev)
    wide[:, 5:5 + m] = c['raw'][:n]
    rows, g = _native(kind, c, 0.25, sub, n, raw=wide[:, 5:5 + m].detach())
    assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])
    buf = torch.zeros(n * m + 1, device=dev)
    buf[1:] = c['raw'][:n].reshape(-1)
    off = buf[1:].view(n, m)
    buf2 = torch.zeros(n * (m // 2) + 1, device=dev)
    buf2[1:] = c['gt_pts'][:n].reshape(-1)
    off2 = buf2[1:].view(n, m // 2)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and off2.data_ptr() % 8 == 4
    rows, g = _native(kind, c, 0.25, sub, n, raw=off.detach(), gt_pts=off2)
    assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])
    wide_w = torch.zeros(n, 4, device=dev)                              # the head's weight: a column of (n, 4)
    wide_w[:, 0] = c['weight'][:n]
    rows, g = _native(kind, c, 0.25, sub, n, weight=wide_w[:, 0])
    assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])
    one = torch.ones((), device=dev)
    rows, g = _native(kind, c, 0.25, sub, n, up=one.expand(n))
    rows2, g2 = _native(kind, c, 0.25, sub, n, up=torch.ones(n, device=dev))
    assert torch.equal(rows, full[:n]) and torch.equal(g, g2)
    rows, g = _native(kind, c, 0.25, sub, n, vs=c['vs'][:n].long())
    assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])


@pytest.mark.parametrize('kind,nv', [('polygon', 36), ('keypoint', 17)])
def test_mismatched_side_tensors_never_reach_the_kernel(kind, nv, monkeypatch):
    from lsnet_amd.ops import cross_iou as fused
    c = _on(lsc.shared_case(kind, nv, 9), _dev())
    c = {k: v[:64] for k, v in c.items()}
    launched = []
    base = dict(pred_raw=c['raw'], gt_pts=c['gt_pts'], anchor3=c['anchor3'], bbox_gt=c['box'], vs=c['vs'], weight=c['weight'])
    assert fused.stage_usable(kind, **base)
    bad = [dict(gt_pts=c['gt_pts'][:-1]), dict(gt_pts=c['gt_pts'][:, :-2]), dict(weight=c['weight'][:-1]),
           dict(anchor3=c['anchor3'][:, :2]), dict(weight=c['weight'].cpu()), dict(gt_pts=c['gt_pts'].double()),
           dict(pred_raw=c['raw'][:, :-2])]
    bad += [dict(bbox_gt=c['box'][:-1]), dict(bbox_gt=None)] if kind == 'polygon' else \
        [dict(vs=c['vs'].cpu()), dict(vs=c['vs'][:, :-1]), dict(vs=None)]
    monkeypatch.setattr(fused._CrossIouStage, 'apply', lambda *a: launched.append(a))
    for change in bad:
        a = dict(base, **change)
        assert not fused.stage_usable(kind, **a), sorted(change)
        with pytest.raises(ValueError):
            fused.cross_iou_stage_rows(kind, a['pred_raw'], a['gt_pts'], a['anchor3'], a['bbox_gt'], a['vs'], a['weight'],
                                       lec.BASE_SCALE, 0.25, 1e-6, 9)
    if kind == 'polygon':
        assert not fused.stage_usable(kind, **base, stride=0) and not fused.stage_usable(kind, **base, stride=17)
    assert not launched


def _spies(monkeypatch):
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    from lsnet_amd.ops import cross_iou as fused
    seen = dict(stage=[], bbox_stage=0, rows=0, passes=0)
    stage, bbox_stage, rows, levels = fused.cross_iou_stage_rows, fused.cross_iou_bbox_stage_rows, fused.cross_iou_rows, \
        LSHead.loss_levels

    def spy_stage(kind, *a, **k):
        seen['stage'].append(kind)
        return stage(kind, *a, **k)

    def spy_bbox(*a, **k):
        seen['bbox_stage'] += 1
        return bbox_stage(*a, **k)

    def spy_rows(*a, **k):
        seen['rows'] += 1
        return rows(*a, **k)

    def spy_levels(self, *a, **k):
        seen['passes'] += 1
        return levels(self, *a, **k)
    monkeypatch.setattr(fused, 'cross_iou_stage_rows', spy_stage)
    monkeypatch.setattr(fused, 'cross_iou_bbox_stage_rows', spy_bbox)
    monkeypatch.setattr(fused, 'cross_iou_rows', spy_rows)
    monkeypatch.setattr(LSHead, 'loss_levels', spy_levels)
    return seen


@pytest.mark.parametrize('switch', ['1', '0'])
@pytest.mark.parametrize('task', ['segm', 'pose_bbox', 'pose_kbox'])
def test_head_route(task, switch, monkeypatch):
    """The golden head fixture with the stage call (init and refine: two calls per evaluation of loss_levels, the bbox branch
    of pose_bbox keeping lsn_cross_iou_bbox_stage) and, with LSNET_CIOU_STAGE=0, on the statements + cross_iou_rows."""
    from tests import golden_cases as gc
    monkeypatch.setenv('LSNET_FUSED_CIOU', '1')
    monkeypatch.setenv('LSNET_CIOU_STAGE', switch)
    seen = _spies(monkeypatch)
    gc.head_case(task, _dev(), channels_last=True)
    kind = 'polygon' if task == 'segm' else 'keypoint'
    passes = seen['passes']
    assert passes >= 1
    assert seen['bbox_stage'] == (2 * passes if task == 'pose_bbox' else 0)
    if switch == '1':
        assert seen['stage'] == [kind] * (2 * passes) and seen['rows'] == 0
    else:
        assert seen['stage'] == [] and seen['rows'] == 2 * passes
