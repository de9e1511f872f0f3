"""Sigmoid focal loss (csrc/misc.hip) and the fused cross-IOU rows (csrc/loss.hip) on the device against float64 statements of
their formulas, at the inputs tests/loss_edge_cases.py builds: saturated logit bands, gamma 0 and fractional, ignored rows, the
second trip of the element-wise grid-stride loops, the coarsening branch of the level sums; negative predictions, planted ties
and rows without an object for the cross-IOU rows, the stage kernel called directly, odd storage.

Rule (tests.cpv_cases.judge; per row for the cross-IOU gradients, loss_edge_cases.judge_rows): the native arm's error against
float64 may be at most twice that of the same formulas in fp32 torch on the device, or 1e-6 where that is larger.

Measured on the MI355X, worst case of each group, error against float64 as (native, torch fp32); the module prints them
again at its end (`-s`):
  focal, |x| in [0, 8)      fwd (2.5e-7, 2.5e-7)  bwd (6.1e-7, 6.1e-7)  sums (1.2e-7, 1.3e-7)  weighted bwd (8.7e-7, 8.4e-7)
  focal, |x| in [8, 30)     fwd (1.3e-7, 9.6e-8)  bwd (1.6e-6, 1.6e-6)  sums (9.8e-8, 1.3e-7)  weighted bwd (1.8e-6, 1.8e-6)
  focal, |x| in [30, 87)    fwd (8.8e-8, 8.8e-8)  bwd (4.6e-8, 4.6e-8)  sums (1.4e-7, 9.4e-8)  weighted bwd (1.0e-7, 1.0e-7)
  focal, |x| in [87, 104)   fwd (8.7e-8, 8.7e-8)  bwd (4.5e-8, 4.5e-8)  sums (6.4e-8, 8.0e-8)  weighted bwd (1.0e-7, 1.0e-7)
  focal, |x| in [104, 200]  fwd (5.2e-8, 5.1e-8)  bwd (4.5e-8, 4.5e-8)  sums (8.5e-8, 5.9e-8)  weighted bwd (1.0e-7, 1.0e-7)
  focal, 6554 x 80          fwd (2.8e-7, 2.8e-7)  bwd (7.5e-7, 6.8e-7)  sums (5.7e-8, 5.7e-8)  weighted bwd (1.0e-6, 1.0e-6)
  focal level sums          sums (1.1e-7, 9.7e-8)  bwd (1.0e-6, 1.0e-6)
  cross-IOU bbox            alpha 0.25: loss (1.8e-7, 1.8e-7)  grad (9.0e-7, 1.0e-6);  alpha 0.2: loss (1.2e-7, 1.4e-7)  grad (6.9e-7, 9.1e-7)
  cross-IOU stage           alpha 0.25: loss (2.2e-7, 2.2e-7)  grad (7.2e-7, 1.3e-6);  alpha 0.2: loss (1.7e-7, 1.7e-7)  grad (8.2e-7, 1.6e-6)
  cross-IOU polygon         alpha 0.25: loss (8.2e-8, 9.8e-8)  grad (6.2e-7, 6.7e-7);  alpha 0.2: loss (9.2e-8, 9.1e-8)  grad (5.9e-7, 7.3e-7)
  cross-IOU keypoint        alpha 0.25: loss (1.7e-7, 2.5e-7)  grad (1.7e-7, 8.2e-7);  alpha 0.2: loss (1.3e-7, 7.0e-8)  grad (2.0e-7, 4.0e-7)
(The focal gradient in [8, 30) carries the cancellation of 1 - p in both fp32 arms alike.)
"""
import ctypes

import pytest
import torch

from tests import loss_edge_cases as lec
from tests.cpv_cases import judge

pytestmark = pytest.mark.gpu

WORST = {}


def note(group, pair):
    a, b = WORST.get(group, (0.0, 0.0))
    WORST[group] = (max(a, pair[0]), max(b, pair[1]))


@pytest.fixture(scope='module', autouse=True)
def worst_pairs():
    yield
    for k, (a, b) in WORST.items():
        print(f'\nWORST {k}: native {a:.2e}  torch fp32 {b:.2e}', end='')
    print()


def _dev():
    return torch.device('cuda:0')


# ---------------------------------------------------------------------------------------------------------------- focal
def _focal_arms(x, t, d, w, gamma, alpha, what, group, up=0.37):
    """forward, backward, both sums and the weighted backward of one (logits, targets) pair: native on the device against the
    float64 statement on the CPU, the fp32 statement on the device as the torch arm; -> the native tensors"""
    from lsnet_amd import ops
    dev = _dev()
    xd, td, dd, wd = x.to(dev), t.to(dev), d.to(dev), w.to(dev)
    ref, gref = lec.focal_statement(x, t, gamma, alpha)
    t32, g32 = lec.focal_statement(xd, td, gamma, alpha, torch.float32)
    xg = xd.clone().requires_grad_()
    out = ops.sigmoid_focal_loss(xg, td, gamma, alpha)
    gout, = torch.autograd.grad(out, xg, dd)
    note(group + ' fwd', judge(out, t32, ref, what + ' fwd'))
    note(group + ' bwd', judge(gout, g32 * dd, gref * d.double(), what + ' bwd'))
    s0 = ops.sigmoid_focal_loss_sum(xg, td, None, gamma, alpha)
    note(group + ' sum', judge(s0.reshape(1), t32.sum().reshape(1), ref.sum().reshape(1), what + ' sum'))
    s = ops.sigmoid_focal_loss_sum(xg, td, wd, gamma, alpha)
    note(group + ' sum', judge(s.reshape(1), (t32 * wd[:, None]).sum().reshape(1), (ref * w.double()[:, None]).sum().reshape(1),
                               what + ' weighted sum'))
    gs, = torch.autograd.grad(s * up, xg)
    note(group + ' bwd_w', judge(gs, g32 * wd[:, None] * up, gref * w.double()[:, None] * up, what + ' weighted bwd'))
    ign = td < 0
    assert ign.any() and not out[ign].any() and not gout[ign].any() and not gs[ign].any(), what     # exactly nothing
    assert torch.isfinite(out).all() and torch.isfinite(gout).all() and torch.isfinite(gs).all(), what
    return out, gout, s, gs


@pytest.mark.parametrize('band', range(len(lec.BANDS)))
@pytest.mark.parametrize('N,C', [(257, 7), (1024, 80)])
def test_focal_in_every_logit_band(N, C, band):
    x, t = lec.focal_case(band, N, C, seed=3)
    g = torch.Generator().manual_seed(7)
    d, w = torch.randn(N, C, generator=g), torch.rand(N, generator=g)
    for gamma in lec.GAMMAS:
        for alpha in lec.ALPHAS:
            _focal_arms(x, t, d, w, gamma, alpha, f'focal {N}x{C} band {lec.BANDS[band]} gamma {gamma} alpha {alpha}',
                        f'focal band {band}')


@pytest.mark.parametrize('gamma,alpha', [(2.0, 0.25), (0.5, 0.5)])
def test_focal_second_trip_of_the_grid_stride_loops(gamma, alpha):
    """6554 x 80 = 2048 x 256 + 32 elements: 32 past the element-wise grids' cap (ew_grid: 2048 blocks of 256) and past the sum
    kernel's 1024 blocks.  The last 64 rows must be, bit for bit, what a call on those 64 rows alone gives."""
    from lsnet_amd import ops
    N, C = 6554, 80
    assert N * C == 2048 * 256 + 32
    x, t = lec.focal_case(0, N, C, seed=4)
    t[-1] = 60                                                     # the positive column of the last row lies in the second trip
    g = torch.Generator().manual_seed(8)
    d, w = torch.randn(N, C, generator=g), torch.rand(N, generator=g)
    out, gout, s, gs = _focal_arms(x, t, d, w, gamma, alpha, f'focal seam gamma {gamma} alpha {alpha}', 'focal seam')
    dev = _dev()
    xt = x[-64:].to(dev).requires_grad_()
    tt, dt, wt = t[-64:].to(dev), d[-64:].to(dev), w[-64:].to(dev)
    out_t = ops.sigmoid_focal_loss(xt, tt, gamma, alpha)
    gout_t, = torch.autograd.grad(out_t, xt, dt)
    gs_t, = torch.autograd.grad(ops.sigmoid_focal_loss_sum(xt, tt, wt, gamma, alpha) * 0.37, xt)
    assert torch.equal(out[-64:], out_t) and torch.equal(gout[-64:], gout_t) and torch.equal(gs[-64:], gs_t)


def _level_blocks(B, num_level, C, per):
    """the launch size of lsn_sigmoid_focal_loss_level_sums at `per` elements per block"""
    return B * sum(-(-n * C // per) for n in num_level)


def _level_arms(B, num_level, C, seed, what, group):
    from lsnet_amd.ops.focal import sigmoid_focal_loss_level_sums
    dev = _dev()
    L, nall = len(num_level), sum(num_level)
    N = B * nall
    x, t = lec.focal_case(0, N, C, seed=seed)
    g = torch.Generator().manual_seed(seed)
    w, up = torch.rand(N, generator=g), torch.randn(L, generator=g)
    lvl = torch.repeat_interleave(torch.arange(L), torch.tensor(num_level)).repeat(B)
    ref, gref = lec.focal_statement(x, t, 2.0, 0.25)
    xd, td, wd = x.to(dev), t.to(dev), w.to(dev)
    t32, g32 = lec.focal_statement(xd, td, 2.0, 0.25, torch.float32)
    xg = xd.clone().requires_grad_()
    got = sigmoid_focal_loss_level_sums(xg, td, wd, B, num_level, 2.0, 0.25)
    ggot, = torch.autograd.grad(got, xg, up.to(dev))
    again = sigmoid_focal_loss_level_sums(xg, td, wd, B, num_level, 2.0, 0.25)
    gagain, = torch.autograd.grad(again, xg, up.to(dev))
    assert got.shape == (L,) and torch.equal(got, again) and torch.equal(ggot, gagain), what
    rows64, rows32 = ref.sum(1) * w.double(), (t32 * wd[:, None]).sum(1)
    ggot = ggot.cpu()
    g32 = (g32 * wd[:, None]).cpu()
    for l in range(L):
        sel = lvl == l
        note(group + ' sums', judge(got[l].reshape(1), rows32[sel.to(dev)].sum().reshape(1), rows64[sel].sum().reshape(1),
                                    f'{what} level {l} sum'))
        note(group + ' bwd', judge(ggot[sel], g32[sel] * up[l], gref[sel] * w.double()[sel, None] * float(up[l]),
                                   f'{what} level {l} bwd'))
    g0 = sigmoid_focal_loss_level_sums(xg, td, None, B, num_level, 2.0, 0.25)
    for l in range(L):
        sel = lvl == l
        note(group + ' sums', judge(g0[l].reshape(1), t32[sel.to(dev)].sum().reshape(1), ref[sel].sum().reshape(1),
                                    f'{what} level {l} unweighted sum'))


def test_focal_level_sums_take_the_coarsening_branch():
    """B = 2, levels [27000, 300, 7], C = 80: 1,070 blocks at 4096 elements per block -- more than the 1024 partial sums -- so
    the launch doubles to 8192 per block and 536 blocks (the benchmark's head, 2 x 22,400 x 80, stays just under: 876).  A small
    call right after it would show a ticket or a partial sum left over."""
    B, num_level, C = 2, [27000, 300, 7], 80
    assert _level_blocks(B, num_level, C, 4096) == 1070 > 1024 >= _level_blocks(B, num_level, C, 8192) == 536
    assert _level_blocks(2, [22400], 80, 4096) == 876
    _level_arms(B, num_level, C, 11, 'focal levels coarse', 'focal levels')
    _level_arms(3, [7, 5], 11, 12, 'focal levels small after coarse', 'focal levels')


def test_focal_level_sums_accept_64_ranges_and_refuse_65():
    from lsnet_amd import _lib
    from lsnet_amd.ops.focal import level_rows_ok
    dev = _dev()
    num_level = [3, 2, 1, 1, 1, 1, 1, 1]
    x = torch.zeros(8 * 10, 5, device=dev)
    assert level_rows_ok(x, 8, num_level)
    _level_arms(8, num_level, 5, 13, 'focal levels 8 x 8', 'focal levels')
    B, num_level = 13, [2, 1, 1, 1, 1]
    nall = sum(num_level)
    x = torch.zeros(B * nall, 5, device=dev)
    assert not level_rows_ok(x, B, num_level) and level_rows_ok(x, 12, num_level)
    t = torch.zeros(B * nall, dtype=torch.int64, device=dev)
    out, gout = torch.full((5,), 7.0, device=dev), torch.full_like(x, 7.0)
    starts = (ctypes.c_int * 6)(0, 2, 3, 4, 5, 6)
    lib = _lib.load()
    rc = lib.lsn_sigmoid_focal_loss_level_sums(x.data_ptr(), t.data_ptr(), None, out.data_ptr(), B, nall, 5, 5, starts, 2.0, 0.25,
                                               _lib.stream())
    assert rc != 0 and b'13 images x 5 levels' in lib.lsn_last_error()
    rc = lib.lsn_sigmoid_focal_loss_backward_levels(x.data_ptr(), t.data_ptr(), None, out.data_ptr(), gout.data_ptr(), B, nall, 5,
                                                    5, starts, 2.0, 0.25, _lib.stream())
    assert rc != 0 and b'13 images x 5 levels' in lib.lsn_last_error()
    torch.cuda.synchronize()
    assert (out == 7).all() and (gout == 7).all()                   # nothing was launched


def test_focal_entry_points_refuse_rows_that_do_not_match():
    """targets / weights / upstream gradients that do not cover the logits raise before the library is called"""
    from lsnet_amd import ops
    from lsnet_amd.ops import get_backend
    dev = _dev()
    x = torch.zeros(9, 5, device=dev)
    t = torch.zeros(9, dtype=torch.int64, device=dev)
    w = torch.ones(9, device=dev)
    with pytest.raises(ValueError):
        ops.sigmoid_focal_loss(x, t[:-1], 2.0, 0.25)
    with pytest.raises(ValueError):
        ops.sigmoid_focal_loss_sum(x, t[:-1], None, 2.0, 0.25)
    with pytest.raises(ValueError):
        ops.sigmoid_focal_loss_sum(x, t, w[:-1], 2.0, 0.25)
    be = get_backend(x)
    with pytest.raises(ValueError):
        be.focal_backward(x, t, torch.ones(9, 4, device=dev), 2.0, 0.25)
    with pytest.raises(ValueError):
        be.focal_backward_weighted(x, t, w[:-1], torch.ones(1, device=dev), 2.0, 0.25)
    with pytest.raises(ValueError):
        be.focal_backward_weighted(x, t.cpu(), w, torch.ones(1, device=dev), 2.0, 0.25)
    with pytest.raises(TypeError):
        ops.sigmoid_focal_loss_sum(x, t.int(), None, 2.0, 0.25)


# ------------------------------------------------------------------------------------------------------------ cross-IOU
def _on(case, dev):
    return {k: v.to(dev) for k, v in case.items()}


def _native_rows(kind, c, alpha, sub=9, vs=None):
    """the fused rows of a case that lies on the device -> (rows, d sum(rows * up) / d pred)"""
    from lsnet_amd.ops import cross_iou as fused
    p = c['pred'].clone().requires_grad_()
    if kind == 'bbox':
        rows = fused.cross_iou_bbox_rows(p, c['target'], c['active'], c['anchor'], c['gt'], c['weight'], alpha, 1e-6)
    else:
        rows = fused.cross_iou_rows(p, c['target'], c['active'], kind, c['anchor'], c['gt'], c['vs'] if vs is None else vs,
                                    c['weight'], alpha, 1e-6, sub)
    g, = torch.autograd.grad(rows, p, c['up'])
    return rows.detach(), g


def _judge_rows_case(kind, case, alpha, sub, got, ggot, what, group):
    ref, gref = lec.rows_statement(kind, case, alpha, torch.float64, sub=sub)
    assert torch.isfinite(ref).all() and torch.isfinite(gref).all(), what          # every row, none masked out
    assert lec.decisions_agree(case['pred'], case['target'], case['active'], alpha), what
    t32, g32 = lec.rows_statement(kind, case, alpha, torch.float32, _dev(), sub=sub)
    note(group + ' loss', judge(got, t32, ref, what + ' loss'))
    note(group + ' grad', lec.judge_rows(ggot, g32, gref, what + ' grad'))
    dead = case['weight'] == 0
    assert dead.any() and not got.cpu()[dead].any() and not ggot.cpu()[dead].any(), what
    return ref, t32


@pytest.mark.parametrize('alpha', [0.25, 0.2])
@pytest.mark.parametrize('seed', [0, 1])
def test_bbox_rows_at_the_edges(seed, alpha, monkeypatch):
    """lsn_cross_iou_bbox_forward / _backward through cross_iou_bbox_rows and through CrossIOULoss (rows with
    reduction_override='none', the reduced loss with avg_factor, a per-row weight)."""
    from lsnet_amd.models.losses import CrossIOULoss
    case = lec.rows_case('bbox', seed, 2000, alpha=alpha)
    c = _on(case, _dev())
    what = f'bbox seed {seed} alpha {alpha}'
    got, ggot = _native_rows('bbox', c, alpha)
    ref, t32 = _judge_rows_case('bbox', case, alpha, 9, got, ggot, what, f'ciou bbox alpha {alpha}')
    monkeypatch.setenv('LSNET_FUSED_CIOU', '1')
    loss = CrossIOULoss(loss_type='bbox', alpha=alpha, loss_weight=1.0)
    kw = dict(anchor_pts=c['anchor'], bbox_gt=c['gt'], pos_inds=c['active'])
    p = c['pred'].clone().requires_grad_()
    rows = loss(p, c['target'], c['weight'], reduction_override='none', **kw)
    total = loss(p, c['target'], c['weight'], avg_factor=7.0, **kw)
    g, = torch.autograd.grad(rows, p, c['up'])
    assert torch.equal(rows, got) and torch.equal(g, ggot)                         # the module took the fused rows
    note(f'ciou bbox alpha {alpha} loss', judge(total.reshape(1), (t32.sum() / 7.0).reshape(1), (ref.sum() / 7.0).reshape(1),
                                                 what + ' reduced'))


@pytest.mark.parametrize('alpha', [0.25, 0.2])
def test_stage_kernel_against_the_head_formulation(alpha):
    """cross_iou_bbox_stage_rows, the default path of LSHead's bbox stages, called directly: against `_gt_reg`, the
    normalisation by 4 x stride and cross_iou_loss in float64.  Rows of zero weight: loss and gradient exactly 0."""
    from lsnet_amd.ops import cross_iou as fused
    case = lec.stage_case(5, 3000, alpha)
    c = _on({k: v for k, v in case.items() if k != 'on_anchor'}, _dev())
    what = f'stage alpha {alpha}'
    ref, gref = lec.stage_statement(case, alpha)
    assert torch.isfinite(ref).all() and torch.isfinite(gref).all()
    assert lec.decisions_agree(case['raw'], *lec.stage_targets(case, torch.float32), alpha)
    t32, g32 = lec.stage_statement(case, alpha, torch.float32, _dev())
    p = c['raw'].clone().requires_grad_()
    rows = fused.cross_iou_bbox_stage_rows(p, c['gt_pts'], c['anchor3'], c['box'], c['weight'], lec.BASE_SCALE, alpha, 1e-6)
    g, = torch.autograd.grad(rows, p, c['up'])
    note(f'ciou stage alpha {alpha} loss', judge(rows, t32, ref, what + ' loss'))
    note(f'ciou stage alpha {alpha} grad', lec.judge_rows(g, g32, gref, what + ' grad'))
    dead = (case['weight'] == 0).to(_dev())
    assert dead.sum() > 500 and not rows[dead].any() and not g[dead].any()


POLY = [(36, 9), (9, 9), (36, 1), (36, 16)]
KEYPOINT_NV = [17, 4, 1]


@pytest.mark.parametrize('alpha', [0.25, 0.2])
@pytest.mark.parametrize('kind,nv,sub', [('polygon', nv, sub) for nv, sub in POLY] + [('keypoint', nv, 9) for nv in KEYPOINT_NV])
def test_polygon_and_keypoint_rows_at_the_edges(kind, nv, sub, alpha):
    seed = 20 + nv + sub if kind == 'polygon' else 40 + nv
    case = lec.rows_case(kind, seed, 1500, nv, alpha)
    if kind == 'polygon' and nv == 36:
        assert lec.equal_extremes(case) >= 1
    c = _on(case, _dev())
    got, ggot = _native_rows(kind, c, alpha, sub)
    _judge_rows_case(kind, case, alpha, sub, got, ggot, f'{kind} nv {nv} sub {sub} alpha {alpha}', f'ciou {kind} alpha {alpha}')
    got_i, ggot_i = _native_rows(kind, c, alpha, sub, vs=c['vs'].long())          # the binding converts int64 visibilities
    assert torch.equal(got, got_i) and torch.equal(ggot, ggot_i)


@pytest.mark.parametrize('variant', ['bbox', 'stage'])
def test_rows_of_odd_shapes_and_storage_equal_the_plain_call(variant):
    """n = 0 / 1 / 257, a column slice of a wider tensor, rows at a 4-byte offset of their buffer (contiguous, but not 16-byte
    aligned: they are copied), an expanded upstream gradient: the same bits as the plain call on fresh tensors."""
    from lsnet_amd.ops import cross_iou as fused
    dev = _dev()
    if variant == 'bbox':
        case = lec.rows_case('bbox', 3, 600)
        keys = ('pred', 'target', 'active', 'anchor', 'gt', 'weight')
        call = lambda a: fused.cross_iou_bbox_rows(*a, 0.25, 1e-6)              # noqa: E731
    else:
        case = lec.stage_case(6, 600)
        keys = ('raw', 'gt_pts', 'anchor3', 'box', 'weight')
        call = lambda a: fused.cross_iou_bbox_stage_rows(*a, lec.BASE_SCALE, 0.25, 1e-6)   # noqa: E731
    c = _on(case, dev)

    def run(n, pred=None, second=None, up=None):
        args = [c[k][:n].clone() for k in keys]
        p = (args[0] if pred is None else pred).requires_grad_()
        args[0] = p
        if second is not None:
            args[1] = second
        rows = call(args)
        g, = torch.autograd.grad(rows, p, c['up'][:n].clone() if up is None else up)
        return rows.detach(), g

    full, gfull = run(600)
    for n in (0, 1, 257):
        rows, g = run(n)
        assert rows.shape == (n,) and g.shape == (n, 20)
        assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])
    n = 257
    wide = torch.zeros(n, 32, device=dev)
    wide[:, 5:25] = c[keys[0]][:n]
    rows, g = run(n, pred=wide[:, 5:25].detach())
    assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])
    buf = torch.zeros(n * 20 + 1, device=dev)
    buf[1:] = c[keys[0]][:n].reshape(-1)
    off = buf[1:].view(n, 20)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    second = None
    if variant == 'bbox':                                             # the target rows as well
        buf2 = torch.zeros(n * 20 + 3, device=dev)
        buf2[3:] = c['target'][:n].reshape(-1)
        second = buf2[3:].view(n, 20)
        assert second.data_ptr() % 16 == 12
    rows, g = run(n, pred=off.detach(), second=second)
    assert torch.equal(rows, full[:n]) and torch.equal(g, gfull[:n])
    one = torch.ones((), device=dev)
    rows, g = run(n, up=one.expand(n))
    rows2, g2 = run(n, up=torch.ones(n, device=dev))
    assert torch.equal(rows, full[:n]) and torch.equal(g, g2)


def test_mismatched_side_tensors_never_reach_the_bbox_kernel(monkeypatch):
    """anchor points that do not cover the rows: CrossIOULoss takes the torch formulation, which raises the ordinary shape
    error; the fused rows are not asked.  (The library's launch log is read as well; it only records dense convolutions.)"""
    from lsnet_amd import _lib
    from lsnet_amd.models.losses import CrossIOULoss
    from lsnet_amd.ops import cross_iou as fused
    monkeypatch.setenv('LSNET_FUSED_CIOU', '1')
    c = _on(lec.rows_case('bbox', 0, 64), _dev())
    calls = []
    monkeypatch.setattr(fused, 'cross_iou_bbox_rows', lambda *a, **k: calls.append(a))
    lib = _lib.load()
    _lib.check(lib.lsn_prof_launch_log(1))
    try:
        with pytest.raises(RuntimeError):
            CrossIOULoss(loss_type='bbox')(c['pred'], c['target'], c['weight'], reduction_override='none',
                                           anchor_pts=c['anchor'][:-1], bbox_gt=c['gt'], pos_inds=c['active'])
        assert lib.lsn_prof_read_launches(None, 0) == 0
    finally:
        _lib.check(lib.lsn_prof_launch_log(0))
    assert not calls
    assert not fused.usable(c['pred'], c['target'], 'bbox', c['active'], c['anchor'][:-1], c['gt'], c['weight'])
    assert not fused.usable(c['pred'], c['target'], 'bbox', c['active'], c['anchor'], c['gt'], c['weight'][:-1])
    assert not fused.usable(c['pred'], c['target'], 'bbox', c['active'], c['anchor'], c['gt'].cpu(), c['weight'])
    assert fused.usable(c['pred'], c['target'], 'bbox', c['active'], c['anchor'], c['gt'], c['weight'])
    with pytest.raises(ValueError):
        fused.cross_iou_bbox_stage_rows(c['pred'], c['target'][:, :10], c['gt'][:, :3], c['gt'][:-1], c['weight'], 4.0)
