"""Inputs and float64 statements of the loss-kernel edge tests (tests/test_loss_edges_host.py, tests/test_loss_edges_gpu.py):
sigmoid focal loss (csrc/misc.hip) and the fused cross-IOU rows (csrc/loss.hip, csrc/cross_iou_row.h).

Focal.  `focal_statement` writes the formulas of the header of misc.hip out (it is NOT autograd through a clamp: below the
FLT_MIN clamp autograd gives 0 where the formulas, like the reference kernel, give -alpha).  The logits come one tensor per band
of |x|, so that a band's error is scaled by that band's own magnitude and the saturated bands are not hidden behind the
ordinary one.

Cross-IOU.  Every value lies on a grid of 1/64 (the stage case: raw predictions on 1/64, pixel offsets in multiples of
stride / 64, strides 8 .. 128), predictions in [-2, 3].  On this grid every comparison of the row function -- p against the
completed target, pos against neg, a box edge against the ground-truth edge -- has exact operands in fp32, so it decides the
same way in fp32 and in float64; `decisions_agree` asserts it for the completed targets, the only operands that carry a
product (alpha x active).  Ties are planted with probability ~0.15 each.  A tie against the INACTIVE half alpha x active is only
planted with alpha = 0.25: 0.2 is not representable, `0.2f * act` and `0.2 * act` differ, and such a tie would exist in one
precision only.  Rows without an object (every 17th: zero targets, zero weight) stay in; one positive prediction per landmark
keeps their 0 / 0 (the reference's own behaviour, not pinned here) away, and the tests assert that the float64 statement is
finite in every row."""
import torch

from lsnet_amd.models.losses.cross_iou_loss import cross_iou_loss
from tests.cpv_cases import judge  # noqa: F401  (the rule of the value comparisons, unchanged)

FLT_MIN = 2.0 ** -126                  # what the kernel's literal 1.17549435e-38f is
LOG_FLT_MIN = -87.33654475055310898657
BANDS = [(0.0, 8.0), (8.0, 30.0), (30.0, 87.0), (87.0, 104.0), (104.0, 200.0)]
# exact logits planted into the band they belong to: 0, the clamp (p == FLT_MIN at -87.3365) and expf's overflow (88.7228)
PLANTED = {0: [0.0, -0.0], 3: [87.33, -87.33, 88.73, -88.73]}
GAMMAS = [2.0, 0.0, 0.5, 1.5]
ALPHAS = [0.25, 0.5, 1.0]


# ---------------------------------------------------------------------------------------------------------------- focal
def focal_statement(x, targets, gamma, alpha, dtype=torch.float64):
    """-> (loss, d loss / d x), both (N, C) in `dtype` on x's device:
         p = 1 / (1 + exp(-x)),  log(1 - p) = -x [x >= 0] - log(1 + exp(x - 2 x [x >= 0]))
         FL = -[t == d] alpha (1 - p)^gamma log(max(p, FLT_MIN)) - [t >= 0, t != d] (1 - alpha) p^gamma log(1 - p)
    and nothing where t < 0."""
    x = x.detach().to(dtype)
    col = torch.arange(x.shape[1], device=x.device)
    t = targets.to(x.device).reshape(-1, 1)
    pos, neg = t == col, (t >= 0) & (t != col)
    p = 1 / (1 + torch.exp(-x))
    xp = (x >= 0).to(dtype)
    log1mp = -x * xp - torch.log(1 + torch.exp(x - 2 * x * xp))
    logp = torch.log(torch.clamp(p, min=FLT_MIN))
    zero = torch.zeros_like(x)
    pw_pos, pw_neg = torch.pow(1 - p, gamma), torch.pow(p, gamma)
    loss = torch.where(pos, -alpha * pw_pos * logp, zero) + torch.where(neg, -(1 - alpha) * pw_neg * log1mp, zero)
    grad = (torch.where(pos, -alpha * pw_pos * (1 - p - p * gamma * logp), zero)
            + torch.where(neg, -(1 - alpha) * pw_neg * (log1mp * (1 - p) * gamma - p), zero))
    return loss, grad


def focal_case(band, N, C, seed):
    """-> logits (N, C) fp32 with |x| in BANDS[band] and random signs, targets (N,) int64 from {-1, 0, ..., C}.  The planted
    logits fill whole rows whose targets walk through the columns, so each is met as a positive and as a negative; rows 0 / 1
    are an ignored (-1) and a background (C) row."""
    g = torch.Generator().manual_seed(1000 * seed + band)
    lo, hi = BANDS[band]
    mag = lo + (hi - lo) * torch.rand(N, C, generator=g)
    if band == len(BANDS) - 1:
        mag[2, 0], mag[2, 1 % C] = lo, hi                          # both ends of the last, closed band
    x = mag * (torch.randint(0, 2, (N, C), generator=g) * 2 - 1).float()
    t = torch.randint(-1, C + 1, (N,), generator=g)
    t[0], t[1] = -1, C
    for k, v in enumerate(PLANTED.get(band, [])):
        x[3 + k] = v
        t[3 + k] = k % C
    assert torch.isfinite(x).all() and lo <= float(x.abs().min()) and float(x.abs().max()) <= hi
    return x, t


# ------------------------------------------------------------------------------------------------------------ cross-IOU
def _grid(g, shape, lo, hi):
    """multiples of 1/64 in [lo, hi]"""
    return torch.randint(int(round(lo * 64)), int(round(hi * 64)) + 1, shape, generator=g).float() / 64


def completed(target, active, alpha):
    """the completed target: the inactive half of every pair is alpha x the active half (in target's dtype)"""
    n, m = target.shape
    t2, a2 = target.reshape(n, -1, 2), active.reshape(n, -1, 2)
    act = torch.where(a2[..., 0], t2[..., 0], t2[..., 1])
    return torch.where(a2, t2, (alpha * act).unsqueeze(-1)).reshape(n, m)


def plant_ties(g, pred, target, active, alpha, inactive_ties):
    """pos == neg within a pair, p == completed target on the active half and (alpha = 0.25 only) on the inactive half, each
    with probability 0.15 per pair; -> the new pred"""
    n, m = pred.shape
    a2 = active.reshape(n, -1, 2)
    p2 = pred.reshape(n, -1, 2).clone()
    pair = torch.rand(n, m // 2, generator=g) < 0.15
    p2[..., 1] = torch.where(pair, p2[..., 0], p2[..., 1])
    tie_a = torch.rand(n, m // 2, generator=g) < 0.15
    tie_i = (torch.rand(n, m // 2, generator=g) < 0.15) & bool(inactive_ties)
    sel = torch.where(a2, tie_a.unsqueeze(-1), tie_i.unsqueeze(-1))
    return torch.where(sel, completed(target, active, alpha).reshape(n, -1, 2), p2).reshape(n, m)


def decisions_agree(pred, target, active, alpha):
    """every p <> completed-target comparison decides the same way in fp32 and in float64"""
    c32 = completed(target.float(), active, alpha)
    c64 = completed(target.double(), active, alpha)
    p32, p64 = pred.float(), pred.double()
    return bool(torch.equal(p32 < c32, p64 < c64) and torch.equal(p32 == c32, p64 == c64))


def tie_counts(pred, target, active, alpha):
    """-> dict of how many ties of each kind the rows hold (the tests assert that none of them is missing)"""
    n, m = pred.shape
    c = completed(target, active, alpha)
    eq = pred == c
    p2 = pred.reshape(n, -1, 2)
    pair = p2[..., 0] == p2[..., 1]
    return dict(active=int((eq & active).sum()), inactive=int((eq & ~active & (c != 0)).sum()), pair=int(pair.sum()),
                pair_on_box=int(pair[:, [0, 3, 4, 7]].sum()) if m == 20 else 0, negative=int((pred < 0).sum()))


def _pairs(g, n, m):
    mag = _grid(g, (n, m // 2), 1 / 64, 3)
    pos = torch.rand(n, m // 2, generator=g) > 0.5
    target = torch.zeros(n, m)
    target[:, 0::2] = torch.where(pos, torch.zeros_like(mag), mag)
    target[:, 1::2] = torch.where(pos, mag, torch.zeros_like(mag))
    active = torch.zeros(n, m, dtype=torch.bool)
    active[:, 0::2], active[:, 1::2] = ~pos, pos
    return target, active


def rows_case(kind, seed, n, nv=4, alpha=0.25):
    """kind 'bbox' (20 components), 'polygon' or 'keypoint' (4 (nv + 1) components) -> dict of fp32 CPU tensors: pred, target,
    active (bool), anchor (n, 2), gt (n, 4), vs (n, nv), weight (n,), up (n,): the upstream gradient of the rows."""
    g = torch.Generator().manual_seed(seed)
    m = 20 if kind == 'bbox' else 4 * (nv + 1)
    pred = _grid(g, (n, m), -2, 3)
    target, active = _pairs(g, n, m)
    anchor = _grid(g, (n, 2), 0, 10)
    c = anchor + _grid(g, (n, 2), -1, 1)
    wh = _grid(g, (n, 2), 0.25, 2)
    gt = torch.cat([c - wh, c + wh], 1)
    vs = (torch.rand(n, nv, generator=g) > 0.3).float() * 2            # COCO visibility 0 / 2
    weight = _grid(g, (n,), 1 / 64, 2)
    up = _grid(g, (n,), -1, 1)
    pred = plant_ties(g, pred, target, active, alpha, alpha == 0.25)
    target[::17] = 0                                                   # rows without an object
    weight[::17] = 0
    pred[::17, 1::4] = pred[::17, 1::4].abs() + 1 / 64                 # ... whose max-sums stay positive: no 0 / 0 (the
    if kind == 'bbox':                                                 # box edges below leave landmark 4 alone)
        # a box edge equal to the ground-truth edge: bx1 (+x of landmark 3), by0 (-y of 0), bx0 (-x of 1), by1 (+y of 2)
        for r0, sel, other, val in ((0, 15, 14, gt[:, 2] - anchor[:, 0]), (1, 0, 1, anchor[:, 1] - gt[:, 1]),
                                    (2, 6, 7, anchor[:, 0] - gt[:, 0]), (3, 9, 8, gt[:, 3] - anchor[:, 1])):
            rows = slice(r0, None, 7)
            pred[rows, sel] = val[rows]
            slack = 1 / 64 if sel > other else 0.0                    # pos must be > neg to win; neg wins an equal pair
            pred[rows, other] = torch.minimum(pred[rows, other], val[rows] - slack)
    if kind == 'keypoint' and m >= 12:
        pred[7, 8:12] = 0.0                                            # a landmark below the eps clamp (the one existing
        target[7, 8:12] = 0.0                                          # exception of tests/test_fused_cross_iou.py)
    return dict(pred=pred, target=target, active=active, anchor=anchor, gt=gt, vs=vs, weight=weight, up=up)


def equal_extremes(case):
    """number of polygon rows in which two vertices share an extreme coordinate of the bounding box"""
    p = case['pred'][:, :-4].double()
    p2 = p.reshape(p.shape[0], -1, 2)
    yx = torch.where(p2[..., 1] > p2[..., 0], p2[..., 1], -p2[..., 0]).reshape(p.shape[0], -1, 2)
    hit = torch.zeros(p.shape[0], dtype=torch.bool)
    for v in (yx[..., 0], yx[..., 1]):
        hit |= ((v == v.min(1, keepdim=True)[0]).sum(1) > 1) | ((v == v.max(1, keepdim=True)[0]).sum(1) > 1)
    return int(hit.sum())


def rows_statement(kind, case, alpha, dtype=torch.float64, device='cpu', sub=9, eps=1e-6):
    """the torch formulation (models/losses/cross_iou_loss.py) in `dtype` -> (weighted loss rows, d sum(rows * up) / d pred)"""
    c = {k: (v.to(device) if v.dtype == torch.bool else v.to(device, dtype)) for k, v in case.items()}
    p = c['pred'].clone().requires_grad_()
    rows = cross_iou_loss(p, c['target'], c['weight'], reduction='none', loss_type=kind, anchor_pts=c['anchor'], bbox_gt=c['gt'],
                          pos_inds=c['active'], vs=c['vs'], alpha=alpha, eps=eps, stride=sub)
    (rows * c['up']).sum().backward()
    return rows.detach(), p.grad


STRIDES = [8., 16., 32., 64., 128.]
BASE_SCALE = 4.0


def stage_case(seed, n, alpha=0.25):
    """The inputs of LSHead's bbox regression stage: raw (n, 20) in stride units, gt_pts (n, 10) extreme points (x, y) in pixels,
    anchor3 (n, 3) = (x, y, stride), box (n, 4), weight (n,), up (n,).  Rows without an object have zero points, box and weight,
    as the target builder leaves them."""
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    g = torch.Generator().manual_seed(seed)
    stride = torch.tensor(STRIDES)[torch.randint(0, 5, (n,), generator=g)][:, None]
    anchor = torch.cat([torch.randint(0, 20, (n, 2), generator=g).float() * stride, stride], 1)
    raw = _grid(g, (n, 20), -2, 3)
    centre = anchor[:, :2] + _grid(g, (n, 2), -1, 1) * stride
    half = _grid(g, (n, 2), 0.25, 2) * stride
    box = torch.cat([centre - half, centre + half], 1)
    ext = torch.stack([centre[:, 0], box[:, 1], box[:, 0], centre[:, 1], centre[:, 0], box[:, 3], box[:, 2], centre[:, 1],
                       centre[:, 0], centre[:, 1]], 1) + _grid(g, (n, 10), -1, 1) * stride
    on_anchor = torch.rand(n, 10, generator=g) < 0.1                   # dx == 0 / dy == 0 exactly: the ">= 0" side
    ext = torch.where(on_anchor, anchor[:, :2].repeat(1, 5), ext)
    obj = torch.rand(n, generator=g) > 0.25
    obj[::17] = False
    weight = _grid(g, (n,), 1 / 64, 2) * obj
    up = _grid(g, (n,), -1, 1)
    ext = torch.where(obj[:, None], ext, torch.zeros_like(ext))
    box = torch.where(obj[:, None], box, torch.zeros_like(box))
    reg, active = LSHead._gt_reg(ext, anchor, weight[:, None].expand(-1, 20))
    raw = plant_ties(g, raw, reg / stride, active, alpha, alpha == 0.25)
    raw[~obj, 1::4] = raw[~obj, 1::4].abs() + 1 / 64                   # no 0 / 0 in rows without an object
    rows = slice(0, None, 7)                                           # bx1 == gt[2]
    val = ((box[:, 2] - anchor[:, 0]) / stride[:, 0])[rows]
    raw[rows, 15] = val
    raw[rows, 14] = torch.minimum(raw[rows, 14], val - 1 / 64)
    return dict(raw=raw, gt_pts=ext, anchor3=anchor, box=box, weight=weight, up=up, on_anchor=on_anchor & obj[:, None])


def stage_targets(case, dtype=torch.float64):
    """-> (target in stride units, active) of a stage case, as LSHead._gt_reg builds them"""
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    a = case['anchor3'].to(dtype)
    reg, active = LSHead._gt_reg(case['gt_pts'].to(dtype), a, case['weight'].to(dtype)[:, None].expand(-1, 20))
    return reg / a[:, 2:3], active


def stage_statement(case, alpha, dtype=torch.float64, device='cpu', eps=1e-6):
    """The head formulation (LSHead.loss_levels): `_gt_reg`, normalisation by 4 x stride, cross_iou_loss, in `dtype`
    -> (weighted loss rows, d sum(rows * up) / d raw)"""
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    c = {k: v.to(device, dtype) for k, v in case.items() if k != 'on_anchor'}
    anchor, stride = c['anchor3'], c['anchor3'][:, 2:3]
    norm = BASE_SCALE * stride
    p = c['raw'].clone().requires_grad_()
    reg, active = LSHead._gt_reg(c['gt_pts'], anchor, c['weight'][:, None].expand(-1, 20))
    rows = cross_iou_loss(p * stride / norm, reg / norm, c['weight'], reduction='none', loss_type='bbox',
                          anchor_pts=anchor[:, :2] / norm, bbox_gt=c['box'] / norm, pos_inds=active, alpha=alpha, eps=eps)
    (rows * c['up']).sum().backward()
    return rows.detach(), p.grad


def judge_rows(native, torch32, ref64, what):
    """The rule of tests.cpv_cases.judge, applied per row to a gradient: the error of a row is max |delta| over the row's max
    |reference|; the native arm's worst row may be at most twice the torch fp32 arm's worst row, or 1e-6 where that is larger.
    Rows whose reference is all zero (zero weight) must be exactly zero.  -> (native error, torch error), printed."""
    ref = ref64.detach().double().cpu()
    nat, t32 = native.detach().double().cpu(), torch32.detach().double().cpu()
    assert nat.shape == ref.shape and torch.isfinite(ref).all(), what
    if ref.numel() == 0:
        return 0.0, 0.0
    scale = ref.abs().amax(1)
    live = scale > 0
    assert not nat[~live].any(), (what, 'rows with a zero reference')
    if not live.any():
        return 0.0, 0.0
    e_n = float(((nat - ref).abs().amax(1)[live] / scale[live]).max())
    e_t = float(((t32 - ref).abs().amax(1)[live] / scale[live]).max())
    print(f'{what}: native {e_n:.3e}  torch fp32 {e_t:.3e}  (rows {int(live.sum())})')
    assert e_n <= max(2 * e_t, 1e-6), (what, e_n, e_t)
    return e_n, e_t
