"""The losses LSCPVHead adds to LSHead as kernels of the library (csrc/cpv.hip): corner heat-map + corner offset of all levels
in one call, and the box-level semantic loss over all levels in one call.  The maps are read in place in whatever memory
format they have; nothing is permuted, concatenated or interpolated first.  Sums are added in a fixed order (no atomics):
the same inputs give the same bits."""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .backend import get_backend

# LSNET_NATIVE_CPV=0: the torch statements of PointHMAssigner and LSCPVHead.loss on the device too (A/B switch; the tests
# compare the two)
NATIVE_CPV = os.environ.get('LSNET_NATIVE_CPV', '1') != '0'
MAX_LEVELS, MAX_IMAGES = 8, 64


def native_ok(*tensors):
    """The library's corner-verification kernels take these tensors (None: an optional one that is absent)."""
    return NATIVE_CPV and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)


class _CornerLossFunction(Function):
    """(loss_heat (L,), loss_off (L,)) of the per-level corner score / offset maps against the targets of
    corner_targets_batch: lsn_corner_loss_forward / _backward, two launches forward and one backward for all levels."""

    @staticmethod
    def forward(ctx, hm, off, valid, npos, alpha, gamma, beta, *maps):
        L = len(maps) // 2
        ctx.cfg = (float(alpha), float(gamma), float(beta))
        ctx.has_valid = valid is not None
        ctx.save_for_backward(hm, off, valid if valid is not None else hm.new_empty(0), npos, *maps)
        heat, offl = get_backend(hm).corner_loss_forward(maps[:L], maps[L:], hm, off, valid, npos, *ctx.cfg)
        return heat, offl

    @staticmethod
    @once_differentiable
    def backward(ctx, g_heat, g_off):
        hm, off, valid, npos, *maps = ctx.saved_tensors
        L = len(maps) // 2
        gs, go = get_backend(hm).corner_loss_backward(maps[:L], maps[L:], hm, off, valid if ctx.has_valid else None, npos,
                                                      *ctx.cfg, g_heat, g_off)
        return (None,) * 7 + tuple(gs) + tuple(go)


def corner_losses(scores, offsets, hm, off, valid, npos, alpha, gamma, beta):
    """scores / offsets: per level (B, 2, H, W) logits / (B, 4, H, W); hm (B, 2, P), off (B, 2, P, 2), npos (B, 2) int32 and
    valid (B, P) or None from corner_targets_batch.  -> (L,) heat-map and (L,) offset losses, normalised per corner by
    sum_img max(n_pos, 1) and averaged over the two corners; loss weights are the caller's."""
    assert len(scores) == len(offsets) <= MAX_LEVELS
    return _CornerLossFunction.apply(hm, off, valid, npos, alpha, gamma, beta, *scores, *offsets)


class _SepFocalFunction(Function):
    """SEPFocalLoss of the per-level semantic logits against the stride-8 maps (lsn_sep_focal_forward / _backward)."""

    @staticmethod
    def forward(ctx, target, weight, gamma, alpha, *logits):
        ctx.cfg = (float(gamma), float(alpha))
        loss, stats = get_backend(target).sep_focal_forward(logits, target, weight, *ctx.cfg)
        ctx.save_for_backward(target, weight, stats, *logits)
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        target, weight, stats, *logits = ctx.saved_tensors
        grads = get_backend(target).sep_focal_backward(logits, target, weight, *ctx.cfg, stats, g)
        return (None,) * 4 + tuple(grads)


def sep_focal_loss(logits, target, weight, gamma, alpha):
    """logits: per level (B, C, H, W); target / weight: (B, C, h, w), read at every level through the nearest rule of
    F.interpolate.  -> scalar sum_pos / sum_pos(w) + sum_neg / count(target > 0); the loss weight is the caller's."""
    assert len(logits) <= MAX_LEVELS
    return _SepFocalFunction.apply(target, weight, gamma, alpha, *logits)
