"""Inputs and float64 statement of the whole-stage polygon / keypoint cross-IOU tests (tests/test_ciou_stage_host.py,
tests/test_ciou_stage_gpu.py): lsn_cross_iou_stage_forward / _backward (csrc/loss.hip) and the stage rows of
csrc/cross_iou_row.h against `_gt_reg`, the normalisation by 4 x stride and cross_iou_loss as LSHead.loss_levels composes them.

Everything lies on the grid of tests/loss_edge_cases.py: raw predictions are multiples of 1/64 in [1/64, 3], anchors integer
multiples of their stride, the offsets gt - anchor multiples of stride / 64 within [-3, 3] x stride, strides 8 .. 128.  Every
scaling by stride and by 4 x stride is therefore exact, and every comparison of the row function -- p against the completed
target, pos against neg, an extreme against another -- has exact operands except the alpha x active product, for which
`decisions_agree` is asserted.  About 40 % of the rows carry no object: zero points, zero box and zero weight, as the target
builder leaves them; their predictions are positive, so the float64 statement is finite there (asserted by the tests)."""
import functools

import torch

from lsnet_amd.models.losses.cross_iou_loss import cross_iou_loss
from tests.loss_edge_cases import BASE_SCALE, STRIDES, _grid

POLY = [(36, 9), (9, 9), (36, 1), (36, 16)]          # (nv, sub)
KEYPOINT_NV = [17, 4, 1]
ALPHAS = [0.25, 0.2]
N_ROWS = 1500
# (kind, nv, sub) of every case
CASES = [('polygon', nv, sub) for nv, sub in POLY] + [('keypoint', nv, 9) for nv in KEYPOINT_NV]


def case_seed(kind, nv, sub):
    return (20 + nv + sub) if kind == 'polygon' else (40 + nv)


def stage_case(kind, nv, n, seed):
    """-> dict of fp32 CPU tensors: raw (n, 4 (nv + 1)) in stride units, gt_pts (n, 2 (nv + 1)) landmarks + centre as (x, y) in
    pixels, anchor3 (n, 3) = (x, y, stride), box (n, 4), vs (n, nv) in {0, 2}, weight (n,), up (n,): the upstream gradient.
    Row 1 (an object row) has dx == 0 exactly on landmark 0; every seventh row ties raw == |d| / stride on active halves."""
    g = torch.Generator().manual_seed(seed)
    m, L = 4 * (nv + 1), nv + 1
    stride = torch.tensor(STRIDES)[torch.randint(0, 5, (n,), generator=g)][:, None]
    anchor = torch.cat([torch.randint(0, 20, (n, 2), generator=g).float() * stride, stride], 1)
    raw = _grid(g, (n, m), 1 / 64, 3)
    off = _grid(g, (n, 2 * L), -3, 3)                                  # (gt - anchor) / stride, (x, y) per landmark
    obj = torch.rand(n, generator=g) > 0.4
    obj[:8] = True
    off[1, 0] = 0.0                                                    # dx == 0 exactly: the ">= 0" side
    pts = anchor[:, :2].repeat(1, L) + off * stride
    xs, ys = pts[:, 0:2 * nv:2], pts[:, 1:2 * nv:2]
    box = torch.stack([xs.min(1)[0], ys.min(1)[0], xs.max(1)[0], ys.max(1)[0]], 1)
    vs = (torch.rand(n, nv, generator=g) > 0.3).float() * 2            # COCO visibility 0 / 2
    weight = _grid(g, (n,), 1 / 64, 2) * obj
    up = _grid(g, (n,), -1, 1)
    # ties on the active half: component [y_up, y_down, x_left, x_right] of landmark k is active where its sign matches d
    plant = (torch.rand(n, 2 * L, generator=g) < 0.5) & (off != 0) & obj[:, None]
    plant[torch.arange(n) % 7 != 0] = False
    r4 = raw.reshape(n, L, 4).clone()
    dx, dy = off[:, 0::2], off[:, 1::2]
    px, py = plant[:, 0::2], plant[:, 1::2]
    r4[..., 0] = torch.where(py & (dy < 0), dy.abs(), r4[..., 0])
    r4[..., 1] = torch.where(py & (dy >= 0), dy.abs(), r4[..., 1])
    r4[..., 2] = torch.where(px & (dx < 0), dx.abs(), r4[..., 2])
    r4[..., 3] = torch.where(px & (dx >= 0), dx.abs(), r4[..., 3])
    raw = r4.reshape(n, m)
    assert float(raw.min()) >= 1 / 64 and float(raw.max()) <= 3 and int(plant.sum()) > 0
    pts = torch.where(obj[:, None], pts, torch.zeros_like(pts))
    box = torch.where(obj[:, None], box, torch.zeros_like(box))
    return dict(raw=raw, gt_pts=pts, anchor3=anchor, box=box, vs=vs, weight=weight, up=up)


@functools.lru_cache(maxsize=None)
def shared_case(kind, nv, sub):
    """the 1,500-row case of (kind, nv, sub), built once per process; read-only"""
    return stage_case(kind, nv, N_ROWS, case_seed(kind, nv, sub))


def stage_targets(case, dtype=torch.float64):
    """-> (target in stride units, active) of a stage case, as LSHead._gt_reg builds them"""
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    a = case['anchor3'].to(dtype)
    width = case['raw'].shape[1]
    reg, active = LSHead._gt_reg(case['gt_pts'].to(dtype), a, case['weight'].to(dtype)[:, None].expand(-1, width))
    return reg / a[:, 2:3], active


def stage_statement(kind, case, alpha, dtype=torch.float64, device='cpu', sub=9, eps=1e-6):
    """The head formulation (LSHead.loss_levels): `_gt_reg`, normalisation by 4 x stride, cross_iou_loss, in `dtype`
    -> (weighted loss rows, d sum(rows * up) / d raw)"""
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    c = {k: v.to(device, dtype) for k, v in case.items()}
    anchor, stride = c['anchor3'], c['anchor3'][:, 2:3]
    norm = BASE_SCALE * stride
    width = c['raw'].shape[1]
    p = c['raw'].clone().requires_grad_()
    reg, active = LSHead._gt_reg(c['gt_pts'], anchor, c['weight'][:, None].expand(-1, width))
    kw = dict(bbox_gt=c['box'] / norm) if kind == 'polygon' else dict(bbox_gt=None, vs=c['vs'])
    rows = cross_iou_loss(p * stride / norm, reg / norm, c['weight'], reduction='none', loss_type=kind,
                          anchor_pts=anchor[:, :2] / norm, pos_inds=active, alpha=alpha, eps=eps, stride=sub, **kw)
    (rows * c['up']).sum().backward()
    return rows.detach(), p.grad


@functools.lru_cache(maxsize=None)
def reference(kind, nv, sub, alpha):
    """the float64 statement of the shared case on the CPU, computed once per process; read-only"""
    return stage_statement(kind, shared_case(kind, nv, sub), alpha, torch.float64, 'cpu', sub)
