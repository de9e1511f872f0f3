"""Fused cross-IOU loss (csrc/loss.hip): the per-point loss and its gradient in one launch each, instead of the ~60
elementwise launches of the torch formulation (models/losses/cross_iou_loss.py) -- the bbox task
(lsn_cross_iou_bbox_forward / _backward and the whole-stage variant), the polygon (instance segmentation) and the
keypoint (pose) tasks (lsn_cross_iou_rows_forward / _backward).  On by default for device tensors (verified on the MI355X against the torch
formulation and the reference fixture: tests/test_zz_fused_ciou_gpu.py; against float64 at negative predictions, ties and odd
storage: tests/test_loss_edges_gpu.py); `LSNET_FUSED_CIOU=0` keeps the torch formulation.  The whole regression stage of the
segm / pose tasks -- scaling, normalisation, target construction and the polygon / keypoint row on an LDS tile -- is
lsn_cross_iou_stage_forward / _backward (cross_iou_stage_rows; tests/test_ciou_stage_gpu.py); `LSNET_CIOU_STAGE=0` keeps LSHead on
the statements around cross_iou_rows."""
import os

import torch

from .. import _lib
from .._lib import ptr, stream


def enabled():
    return os.environ.get('LSNET_FUSED_CIOU', '1') != '0'


def _rows16(t):
    """`t` as contiguous rows at a 16-byte aligned address, as the bbox / stage kernels' float4 accesses need them.
    `.contiguous()` leaves a contiguous view at an odd element offset (buf[1:].view(n, 20)) where it is: that one is copied."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def shapes_match(pred, want):
    """`want`: (tensor or None, shape) pairs.  True when every tensor given has its shape and lies on pred's device.  The
    kernels index their side tensors unchecked, so this is what keeps a short buffer away from them."""
    return all(t is None or (tuple(t.shape) == tuple(shape) and t.device == pred.device) for t, shape in want)


class _CrossIouBbox(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pred, target, active, anchor, bbox_gt, weight, alpha, eps):
        pred, target = _rows16(pred), _rows16(target)
        active = active.to(torch.uint8).contiguous()
        anchor, bbox_gt = anchor.contiguous(), bbox_gt.contiguous()
        weight = None if weight is None else weight.contiguous()
        loss = torch.empty(pred.shape[0], dtype=torch.float32, device=pred.device)
        _lib.check(_lib.load().lsn_cross_iou_bbox_forward(ptr(pred), ptr(target), ptr(active), ptr(anchor), ptr(bbox_gt),
                                                          ptr(weight), pred.shape[0], alpha, eps, ptr(loss), stream()))
        ctx.save_for_backward(pred, target, active, anchor, bbox_gt, *([weight] if weight is not None else []))
        ctx.cfg = (alpha, eps, weight is not None)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rows):
        alpha, eps, has_w = ctx.cfg
        pred, target, active, anchor, bbox_gt, *rest = ctx.saved_tensors
        weight = rest[0] if has_w else None
        grad = torch.empty_like(pred)
        _lib.check(_lib.load().lsn_cross_iou_bbox_backward(ptr(pred), ptr(target), ptr(active), ptr(anchor), ptr(bbox_gt),
                                                           ptr(weight), ptr(grad_rows.contiguous()), pred.shape[0], alpha, eps,
                                                           ptr(grad), stream()))
        return grad, None, None, None, None, None, None, None


def usable(pred, target, loss_type, active=None, anchor=None, bbox_gt=None, weight=None):
    """The bbox kernels: rows of 20 fp32 components on the device, with every side tensor they index (active[20 i],
    anchor[2 i], bbox_gt[4 i], weight[i]) present and of matching shape.  A mismatch sends the caller to the torch formulation,
    which raises the ordinary shape error."""
    if not (loss_type == 'bbox' and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 2
            and pred.shape[1] == 20 and not target.requires_grad):
        return False
    if active is None or anchor is None or bbox_gt is None:
        return False
    n = pred.shape[0]
    return shapes_match(pred, ((target, (n, 20)), (active, (n, 20)), (anchor, (n, 2)), (bbox_gt, (n, 4)), (weight, (n,))))


_KIND = {'polygon': 1, 'keypoint': 2}


def rows_usable(pred, target, loss_type, stride=9, active=None, anchor=None, bbox_gt=None, vs=None, weight=None):
    """The polygon / keypoint kernels: rows of 4 (nv + 1) fp32 components on the device.  The kernels index the side
    tensors unchecked (active[M i], anchor[2 i], bbox_gt[4 i], vs[(M / 4 - 1) i], weight[i]): every tensor handed in is
    verified here -- shape, device -- and a mismatch sends the caller to the torch formulation, which raises the shape
    error a user expects instead of reading out of bounds."""
    if not (loss_type in _KIND and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 2
            and pred.shape[1] >= 8 and pred.shape[1] % 4 == 0 and not target.requires_grad
            and (loss_type == 'keypoint' or 1 <= stride <= min(16, pred.shape[1] // 4))):
        return False
    n, m = pred.shape
    return shapes_match(pred, ((target, (n, m)), (active, (n, m)), (anchor, (n, 2)), (bbox_gt, (n, 4)), (vs, (n, m // 4 - 1)),
                               (weight, (n,))))


class _CrossIouRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pred, target, active, anchor, bbox_gt, vs, weight, kind, sub, alpha, eps):
        c = lambda t: None if t is None else t.contiguous()
        pred, target, anchor, bbox_gt, weight = c(pred), c(target), c(anchor), c(bbox_gt), c(weight)
        vs = None if vs is None else vs.to(torch.float32).contiguous()
        active = active.to(torch.uint8).contiguous()
        n, m = pred.shape
        loss = torch.empty(n, dtype=torch.float32, device=pred.device)
        _lib.check(_lib.load().lsn_cross_iou_rows_forward(kind, ptr(pred), ptr(target), ptr(active), ptr(anchor), ptr(bbox_gt),
                                                          ptr(vs), ptr(weight), n, m, sub, alpha, eps, ptr(loss), stream()))
        ctx.save_for_backward(pred, target, active, anchor, bbox_gt, vs, weight)   # (None entries are allowed)
        ctx.cfg = (kind, sub, alpha, eps)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rows):
        kind, sub, alpha, eps = ctx.cfg
        pred, target, active, anchor, bbox_gt, vs, weight = ctx.saved_tensors
        n, m = pred.shape
        grad = torch.empty_like(pred)
        _lib.check(_lib.load().lsn_cross_iou_rows_backward(kind, ptr(pred), ptr(target), ptr(active), ptr(anchor), ptr(bbox_gt),
                                                           ptr(vs), ptr(weight), ptr(grad_rows.contiguous()), n, m, sub, alpha, eps,
                                                           ptr(grad), stream()))
        return (grad,) + (None,) * 10


def cross_iou_rows(pred, target, active, loss_type, anchor=None, bbox_gt=None, vs=None, weight=None, alpha=0.2, eps=1e-6,
                   stride=9):
    """(n,) weighted loss rows (reduction 'none') of the polygon / keypoint cross-IOU loss; gradient flows to `pred` only
    (the other inputs are targets; they are kept alive for the backward launch)."""
    return _CrossIouRows.apply(pred, target, active, anchor, bbox_gt, vs, weight, _KIND[loss_type], int(stride), float(alpha),
                               float(eps))


def cross_iou_bbox_rows(pred, target, active, anchor, bbox_gt, weight=None, alpha=0.2, eps=1e-6):
    """(n,) weighted loss rows (reduction 'none') of the bbox cross-IOU loss; gradient flows to `pred` only."""
    return _CrossIouBbox.apply(pred, target, active, anchor, bbox_gt, weight, float(alpha), float(eps))


class _CrossIouBboxStage(torch.autograd.Function):

    @staticmethod
    def forward(ctx, raw, gt_pts, anchor3, bbox_gt, weight, base, alpha, eps):
        raw, gt_pts, anchor3 = _rows16(raw), gt_pts.contiguous(), anchor3.contiguous()
        bbox_gt, weight = bbox_gt.contiguous(), weight.contiguous()
        loss = torch.empty(raw.shape[0], dtype=torch.float32, device=raw.device)
        _lib.check(_lib.load().lsn_cross_iou_bbox_stage_forward(ptr(raw), ptr(gt_pts), ptr(anchor3), ptr(bbox_gt), ptr(weight),
                                                                raw.shape[0], base, alpha, eps, ptr(loss), stream()))
        ctx.save_for_backward(raw, gt_pts, anchor3, bbox_gt, weight)
        ctx.cfg = (base, alpha, eps)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rows):
        base, alpha, eps = ctx.cfg
        raw, gt_pts, anchor3, bbox_gt, weight = ctx.saved_tensors
        grad = torch.empty_like(raw)
        _lib.check(_lib.load().lsn_cross_iou_bbox_stage_backward(ptr(raw), ptr(gt_pts), ptr(anchor3), ptr(bbox_gt), ptr(weight),
                                                                 ptr(grad_rows.contiguous()), raw.shape[0], base, alpha, eps,
                                                                 ptr(grad), stream()))
        return grad, None, None, None, None, None, None, None


def stage_enabled():
    """`LSNET_CIOU_STAGE=0` keeps the segm / pose stages of LSHead.loss_levels on the torch statements + cross_iou_rows."""
    return os.environ.get('LSNET_CIOU_STAGE', '1') != '0'


STAGE_TILE_ROWS = 64       # rows per workgroup of lsn_cross_iou_stage_* (csrc/loss.hip: CIOU_TILE_ROWS)


def stage_tile_fits(kind, m):
    """csrc/loss.hip, CiouTile: a tile of m-wide rows (predictions, points, the keypoint kind's visibilities at odd pitches, four
    values per row) within 64 KiB of LDS -- polygon rows up to 164 components, keypoint rows up to 140"""
    nv = m // 4 - 1
    return STAGE_TILE_ROWS * 4 * ((m + 1) + (m // 2 + 1) + ((nv | 1) if kind == 'keypoint' else 0) + 4) <= 64 * 1024


def stage_usable(kind, pred_raw, gt_pts, anchor3, bbox_gt, vs, weight, stride=9):
    """The whole-stage polygon / keypoint kernels: rows of 4 (nv + 1) fp32 components on the device whose tile fits the
    kernel's LDS, with every side tensor they index unchecked (gt_pts[2 (nv + 1) i], anchor3[3 i], bbox_gt[4 i], vs[nv i],
    weight[i]) present, fp32 (vs: any dtype, it is converted), of matching shape and on the same device."""
    if not (kind in _KIND and pred_raw.is_cuda and pred_raw.dtype == torch.float32 and pred_raw.dim() == 2
            and pred_raw.shape[1] >= 8 and pred_raw.shape[1] % 4 == 0 and stage_tile_fits(kind, pred_raw.shape[1])):
        return False
    n, m = pred_raw.shape
    nv = m // 4 - 1
    if kind == 'polygon':
        if bbox_gt is None or not (1 <= stride <= min(16, m // 4)):
            return False
    elif vs is None:
        return False
    if gt_pts is None or anchor3 is None or weight is None:
        return False
    if any(t.dtype != torch.float32 or t.requires_grad for t in (gt_pts, anchor3, weight, bbox_gt) if t is not None):
        return False
    return shapes_match(pred_raw, ((gt_pts, (n, m // 2)), (anchor3, (n, 3)), (weight, (n,)),
                                   (bbox_gt if kind == 'polygon' else None, (n, 4)), (vs if kind == 'keypoint' else None, (n, nv))))


class _CrossIouStage(torch.autograd.Function):

    @staticmethod
    def forward(ctx, raw, gt_pts, anchor3, bbox_gt, vs, weight, kind, sub, base, alpha, eps):
        c = lambda t: None if t is None else t.contiguous()       # noqa: E731
        raw, gt_pts, anchor3, bbox_gt, weight = _rows16(raw), _rows16(gt_pts), c(anchor3), c(bbox_gt), c(weight)
        vs = None if vs is None else vs.to(torch.float32).contiguous()
        n, m = raw.shape
        loss = torch.empty(n, dtype=torch.float32, device=raw.device)
        _lib.check(_lib.load().lsn_cross_iou_stage_forward(kind, ptr(raw), ptr(gt_pts), ptr(anchor3), ptr(bbox_gt), ptr(vs),
                                                           ptr(weight), n, m, sub, base, alpha, eps, ptr(loss), stream()))
        ctx.save_for_backward(raw, gt_pts, anchor3, bbox_gt, vs, weight)   # (None entries are allowed)
        ctx.cfg = (kind, sub, base, alpha, eps)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rows):
        kind, sub, base, alpha, eps = ctx.cfg
        raw, gt_pts, anchor3, bbox_gt, vs, weight = ctx.saved_tensors
        n, m = raw.shape
        grad = torch.empty_like(raw)
        _lib.check(_lib.load().lsn_cross_iou_stage_backward(kind, ptr(raw), ptr(gt_pts), ptr(anchor3), ptr(bbox_gt), ptr(vs),
                                                            ptr(weight), ptr(grad_rows.contiguous()), n, m, sub, base, alpha, eps,
                                                            ptr(grad), stream()))
        return (grad,) + (None,) * 10


def cross_iou_stage_rows(kind, pred_raw, gt_pts, anchor3, bbox_gt, vs, weight, base_scale, alpha=0.2, eps=1e-6, stride=9):
    """A regression stage of LSHead's segm (`kind` 'polygon') or pose ('keypoint') task for n points in one launch (see
    lsn_cross_iou_stage_forward): weighted loss rows; gradient flows to `pred_raw`.  `stride`: the polygon kind's number of
    interleaved landmark subsets (CrossIOULoss.stride).  The side tensor the kind does not use (vs / bbox_gt) is ignored."""
    if not stage_usable(kind, pred_raw, gt_pts, anchor3, bbox_gt, vs, weight, stride):
        shape = lambda t: None if t is None else (tuple(t.shape), str(t.device), str(t.dtype))      # noqa: E731
        raise ValueError(f'cross_iou_stage_rows: {kind!r} rows {shape(pred_raw)} beside points {shape(gt_pts)}, anchors '
                         f'{shape(anchor3)}, boxes {shape(bbox_gt)}, visibilities {shape(vs)}, weights {shape(weight)} '
                         f'and {stride} subsets')
    polygon = kind == 'polygon'
    return _CrossIouStage.apply(pred_raw, gt_pts, anchor3, bbox_gt if polygon else None, None if polygon else vs, weight,
                                _KIND[kind], int(stride), float(base_scale), float(alpha), float(eps))


def cross_iou_bbox_stage_rows(pred_raw, gt_pts, anchor3, bbox_gt, weight, base_scale, alpha=0.2, eps=1e-6):
    """The bbox regression stage of LSHead for n points in one launch (see lsn_cross_iou_bbox_stage_forward): weighted
    loss rows; gradient flows to `pred_raw`."""
    n = pred_raw.shape[0]
    if pred_raw.dim() != 2 or pred_raw.shape[1] != 20 or not shapes_match(
            pred_raw, ((gt_pts, (n, 10)), (anchor3, (n, 3)), (bbox_gt, (n, 4)), (weight, (n,)))):
        raise ValueError(f'cross_iou_bbox_stage_rows: {tuple(pred_raw.shape)} predictions beside points {tuple(gt_pts.shape)}, '
                         f'anchors {tuple(anchor3.shape)}, boxes {tuple(bbox_gt.shape)} and weights {tuple(weight.shape)}')
    return _CrossIouBboxStage.apply(pred_raw, gt_pts, anchor3, bbox_gt, weight, float(base_scale), float(alpha), float(eps))
