"""LSHead's point decoding: the pixel-wise statements between the head's 1x1 outputs and their consumers.

  point_decode   raw init output -> (sp, off): sp = softplus(raw[:n_sp]), off = the 2 x taps sampling offsets (signed selection
                 of the picked vectors, the free channels, the gradient_mul mix, minus the base grid);
  softplus_add   softplus(a + b) with b detached: the refine stage's sum with the init prediction;
  point_boxes    the proposal boxes of the refine-stage assignment, all levels and images at once.

On the device these are kernels of the library (lsn_point_decode_* / lsn_softplus_add_* / lsn_point_boxes: csrc/points.hip,
arithmetic and its rounding in csrc/point_rows.h), one launch per pass, and return the bits of the torch statements they
replace.  They take CUDA fp32 tensors of pixel rows: the (B, C, N, 1) channels-last tensors of LSHead._cat_px, their
(B, N, C) row views, or plain (R, C) rows.  Anything else -- host tensors, other dtypes and layouts, LSNET_NATIVE_POINTS=0 --
runs torch statements: the head keeps its own (models/dense_heads/ls_head.py; the tests compare the two), the functions here
state the same arithmetic for any table of offset sources."""
import math
import os

import torch
import torch.nn.functional as F

from .backend import get_backend

# LSNET_NATIVE_POINTS=0: the torch statements on the device too (A/B switch; tools/README.md)
NATIVE_POINTS = os.environ.get('LSNET_NATIVE_POINTS', '1') != '0'
MAX_RAW, MAX_OFF = 256, 32       # what the kernels' tables hold (csrc/points.hip)


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def row_layout(t):
    """(row pitch in floats, rows, row width) when `t` is a tensor of pixel rows the kernels address by (base, pitch): a
    (B, C, N, 1) tensor with channels innermost, a (B, N, C) tensor or (R, C) rows -- dense, or column slices of dense ones --
    else None.  (Strides of extent-1 axes say nothing.)"""
    if t.numel() == 0:
        return None
    if t.dim() == 4 and t.shape[3] == 1:
        B, C, N = t.shape[:3]
        sb, sc, sn = t.stride()[:3]
    elif t.dim() == 3:
        B, N, C = t.shape
        sb, sn, sc = t.stride()
    elif t.dim() == 2:
        (N, C), B = t.shape, 1
        (sn, sc), sb = t.stride(), 0
    else:
        return None
    if C > 1 and sc != 1:
        return None
    pitch = sn if N > 1 else sb if B > 1 else C
    if pitch < C or (B > 1 and sb != N * pitch):
        return None
    return pitch, B * N, C


def rows_like(t, width):
    """a new dense tensor of `t`'s form (see row_layout) with rows of `width` floats"""
    if t.dim() == 4:
        return t.new_empty((t.shape[0], t.shape[2], width)).unsqueeze(2).permute(0, 3, 1, 2)
    return t.new_empty(tuple(t.shape[:-1]) + (width,))


def _dense_rows(t):
    """`t` as the kernels read it (autograd may hand a gradient over in any layout)"""
    if t.dtype == torch.float32 and row_layout(t) is not None:
        return t
    t = t.float()
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t.contiguous()


def native_ok(*tensors):
    """The library's point kernels take these tensors: CUDA fp32 pixel rows."""
    if not NATIVE_POINTS:
        return False
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and row_layout(t) is not None for t in tensors)


# ---- the table of offset sources ---------------------------------------------------------------------------------------------
def offset_sources(task, n_sp, c_raw, num_kernel_points=9):
    """Where each of the 2 x taps offset channels of a branch comes from, as `get_pred_reg` selects them: entry j = 2 t + comp
    (comp 0: y, 1: x) >= 0 is the sp channel 4 v + 2 comp of the (neg, pos) pair of picked vector v = pick[t]; entry -1 - i is
    the free channel raw[n_sp + i].  A branch with free channels (the bbox branch) picks all its vectors; otherwise the picks
    are every ceil(nv / 8)-th contour vector (task 'segm') or every second keypoint from 1 on (pose), then the centre vector."""
    n_vec = n_sp // 4
    if c_raw > n_sp:
        picks = list(range(n_vec))
    else:
        nv = n_vec - 1
        picks = list(range(0, nv, math.ceil(nv / (num_kernel_points - 1)))) if task == 'segm' else list(range(1, nv, 2))
        picks.append(nv)
    return tuple(4 * v + 2 * comp for v in picks for comp in (0, 1)) + tuple(-1 - i for i in range(c_raw - n_sp))


def _table_ok(picks, n_sp, c_raw):
    seen = set()
    for s in picks:
        key = s if s >= 0 else n_sp - 1 - s
        if key in seen or not ((s >= 0 and s % 2 == 0 and s + 1 < n_sp) or (s < 0 and key < c_raw)):
            return False
        seen.add(key)
    return 0 < len(picks) <= MAX_OFF and n_sp % 4 == 0 and 0 < n_sp <= c_raw <= MAX_RAW


def _signed(neg, pos):
    return torch.where(pos > neg, pos, -neg)


def _channels(t, idx):
    dim = 1 if t.dim() == 4 else t.dim() - 1
    return t.index_select(dim, torch.as_tensor(idx, dtype=torch.long, device=t.device))


def point_decode_torch(raw, n_sp, picks, gradient_mul, base):
    """The torch statements of point_decode for any table (the head's own are LSHead.forward's)."""
    dim = 1 if raw.dim() == 4 else raw.dim() - 1
    sp = F.softplus(raw.narrow(dim, 0, n_sp))
    cols = []
    for s in picks:
        if s >= 0:
            cols.append(_signed(sp.narrow(dim, s, 1), sp.narrow(dim, s + 1, 1)))
        else:
            cols.append(raw.narrow(dim, n_sp - 1 - s, 1))
    reg = torch.cat(cols, dim=dim)
    reg = (1 - gradient_mul) * reg.detach() + gradient_mul * reg
    shape = [1] * raw.dim()
    shape[dim] = len(picks)
    return sp, reg - base.reshape(-1)[:len(picks)].to(reg.dtype).view(shape)


# ---- point decode ------------------------------------------------------------------------------------------------------------
class _PointDecodeFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, raw, n_sp, picks, gradient_mul, base):
        sp, off = get_backend(raw).point_decode_forward(raw, n_sp, picks, gradient_mul, base)
        ctx.cfg = (n_sp, picks, gradient_mul)
        ctx.set_materialize_grads(False)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(raw, sp)
        return sp, off

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sp, g_off):
        if not ctx.needs_input_grad[0] or (g_sp is None and g_off is None):
            return None, None, None, None, None
        raw, sp = ctx.saved_tensors
        n_sp, picks, gradient_mul = ctx.cfg
        g_sp = None if g_sp is None else _dense_rows(g_sp)
        g_off = None if g_off is None else _dense_rows(g_off)
        g_raw = get_backend(raw).point_decode_backward(raw, sp, n_sp, picks, gradient_mul, g_sp, g_off)
        return g_raw, None, None, None, None


def point_decode(raw, n_sp, picks, gradient_mul, base):
    """raw: the init 1x1's output as pixel rows of c_raw channels; picks: the table of `offset_sources`; base: the base grid
    (at least len(picks) values, (y, x) per tap).  Returns (sp, off) in raw's form: sp = softplus(raw[:n_sp]),
    off[j] = ((1 - gm) * s.detach() + gm * s) - base[j] with s the signed pair or free channel picks[j] names."""
    picks = tuple(int(s) for s in picks)
    lay = row_layout(raw)
    if native_ok(raw) and lay is not None and _table_ok(picks, n_sp, lay[2]) and torch.is_tensor(base) and base.is_cuda:
        base32 = base if base.dtype == torch.float32 and base.is_contiguous() else base.float().contiguous()
        return _PointDecodeFn.apply(raw, int(n_sp), picks, float(gradient_mul), base32)
    return point_decode_torch(raw, n_sp, picks, gradient_mul, base)


# ---- softplus(a + b) ---------------------------------------------------------------------------------------------------------
class _SoftplusAddFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, a, b):
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(a, b)
        return get_backend(a).softplus_add_forward(a, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        a, b = ctx.saved_tensors
        return get_backend(a).softplus_add_backward(a, b, _dense_rows(g)), None


def softplus_add(a, b_detached):
    """softplus(a + b) (beta 1, threshold 20); the gradient goes to a only."""
    b = b_detached.detach()
    if native_ok(a, b) and a.shape == b.shape:
        return _SoftplusAddFn.apply(a, b)
    return F.softplus(a + b)


# ---- proposal boxes ----------------------------------------------------------------------------------------------------------
def boxes_ok(rows, flat_points):
    return native_ok(rows) and rows.dim() == 3 and torch.is_tensor(flat_points) and flat_points.is_cuda \
        and flat_points.dtype == torch.float32 and flat_points.is_contiguous() \
        and tuple(flat_points.shape) == (rows.shape[1], 3)


def point_boxes_torch(rows, flat_points, mode, nv):
    B, N, _ = rows.shape
    n = 4 if mode == 'extreme' else nv
    v = rows[:, :, :4 * n].reshape(B, N, n, 2, 2)
    v = _signed(v[..., 0], v[..., 1])                                        # (B, N, n, [y, x])
    y, x = v[..., 0], v[..., 1]
    if mode == 'extreme':
        box = torch.stack([x[..., 1], y[..., 0], x[..., 3], y[..., 2]], dim=-1)
    else:
        box = torch.stack([x.min(-1)[0], y.min(-1)[0], x.max(-1)[0], y.max(-1)[0]], dim=-1)
    xy = flat_points[:, :2]
    return torch.cat([xy, xy], dim=1)[None] + box * flat_points[None, :, 2:3]


def point_boxes(rows, flat_points, mode, nv):
    """rows: the (detached) init predictions of the box branch as (B, N_all, C) rows; flat_points (N_all, 3) = x, y, stride.
    mode 'extreme': the box of landmarks (top, left, bottom, right), as extreme_points2bbox; 'vectors': the bounding box of
    the first nv vectors, as vectors2bbox.  Returns point + box * stride, (B, N_all, 4)."""
    assert mode in ('extreme', 'vectors'), mode
    rows = rows.detach()
    if boxes_ok(rows, flat_points) and rows.shape[2] >= (16 if mode == 'extreme' else 4 * nv) and nv > 0:
        return get_backend(rows).point_boxes(rows, flat_points, mode, nv)
    return point_boxes_torch(rows, flat_points, mode, nv)
