"""The generators and float64 statements of tests/loss_edge_cases.py, pinned on the CPU before anything touches a GPU:
the focal statement against its closed form and its clamp, and the cross-IOU edge rows (negative predictions, planted ties,
rows without an object) through the host-compiled row functions of csrc/cross_iou_row.h, judged against float64 by the rule of
tests.cpv_cases.judge (values) and its per-row form (gradients).  The library of the row functions is the one
tests/test_fused_cross_iou.py compiles."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_edge_cases as lec
from tests.cpv_cases import judge
from tests.test_fused_cross_iou import rowlib  # noqa: F401  (fixture: DRIVER compiled with g++)

F32, U8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)


def _f(t):
    a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
    return a, a.ctypes.data_as(F32)


def _u(t):
    a = np.ascontiguousarray(t.numpy().astype(np.uint8))
    return a, a.ctypes.data_as(U8)


# ---------------------------------------------------------------------------------------------------------------- focal
@pytest.mark.parametrize('gamma', lec.GAMMAS)
@pytest.mark.parametrize('alpha', lec.ALPHAS)
def test_focal_statement_is_the_closed_form_below_87(gamma, alpha):
    """float64, |x| < 87 (no clamp): -alpha (1 - p)^gamma logsigmoid(x) on the positive column, -(1 - alpha) p^gamma
    logsigmoid(-x) on the negative ones, nothing on ignored rows; the gradient against autograd of that form."""
    for band in (0, 1, 2):
        x32, t = lec.focal_case(band, 257, 7, seed=1)
        loss, grad = lec.focal_statement(x32, t, gamma, alpha)
        x = x32.double().requires_grad_()
        col = torch.arange(7)
        pos, neg = t[:, None] == col, (t[:, None] >= 0) & (t[:, None] != col)
        p = torch.sigmoid(x)
        # 1 - p as sigmoid(-x): the closed form must not lose 1 - p to cancellation where the statement's 1 - p is exact enough
        closed = (torch.where(pos, -alpha * torch.pow(1 - p, gamma) * F.logsigmoid(x), torch.zeros_like(x))
                  + torch.where(neg, -(1 - alpha) * torch.pow(p, gamma) * F.logsigmoid(-x), torch.zeros_like(x)))
        scale = float(closed.detach().abs().max())
        assert float((loss - closed.detach()).abs().max()) <= 1e-12 * scale
        up = torch.rand(257, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        if gamma in (0.5, 1.5) and band > 0:
            continue        # autograd of pow at 1 - p == 0 (x > 37 in float64) is inf x 0: the value is checked, the gradient below
        g, = torch.autograd.grad(closed, x, up)
        assert float((grad * up - g).abs().max()) <= 1e-10 * float(g.abs().max())
        assert not loss[t < 0].any() and not grad[t < 0].any()


def test_focal_statement_below_the_clamp_is_what_the_reference_kernel_gives():
    """x < -87.34: p < FLT_MIN, the positive column's loss is alpha x 87.3365 and its gradient -alpha (autograd through a clamp
    would say 0)."""
    x = torch.tensor([[-87.4, -95.0, -104.0, -150.0, -200.0]])
    for alpha in lec.ALPHAS:
        for gamma in lec.GAMMAS:
            for col in range(5):
                loss, grad = lec.focal_statement(x, torch.tensor([col]), gamma, alpha)
                assert abs(float(loss[0, col]) - alpha * -lec.LOG_FLT_MIN) < 1e-12
                assert abs(float(grad[0, col]) + alpha) < 1e-12
    assert abs(np.log(lec.FLT_MIN) - lec.LOG_FLT_MIN) < 1e-13 and np.float32(1.17549435e-38) == lec.FLT_MIN


@pytest.mark.parametrize('band', range(len(lec.BANDS)))
def test_focal_fp32_evaluation_is_finite_in_every_band(band):
    for N, C in ((257, 7), (1024, 80)):
        x, t = lec.focal_case(band, N, C, seed=2)
        assert (t == -1).any() and (t == C).any() and ((t >= 0) & (t < C)).any()
        for gamma in lec.GAMMAS:
            for alpha in lec.ALPHAS:
                for dtype in (torch.float32, torch.float64):
                    loss, grad = lec.focal_statement(x, t, gamma, alpha, dtype)
                    assert torch.isfinite(loss).all() and torch.isfinite(grad).all(), (band, gamma, alpha, dtype)


# ------------------------------------------------------------------------------------------------------------ cross-IOU
def host_rows(lib, kind, case, alpha, sub=9, eps=1e-6):
    """the host-compiled row functions -> (weighted loss rows, gradient of sum(rows * up)) as fp32 tensors"""
    n, m = case['pred'].shape
    loss, grad = np.zeros(n, np.float32), np.zeros((n, m), np.float32)
    arrs = [_f(case[k]) for k in ('pred', 'target', 'anchor', 'gt', 'vs')]
    act = _u(case['active'])
    if kind == 'bbox':
        lib.rows(arrs[0][1], arrs[1][1], act[1], arrs[2][1], arrs[3][1], n, ctypes.c_float(alpha), ctypes.c_float(eps),
                 loss.ctypes.data_as(F32), grad.ctypes.data_as(F32))
    else:
        lib.gen_rows(1 if kind == 'polygon' else 2, arrs[0][1], arrs[1][1], act[1], arrs[2][1], arrs[3][1], arrs[4][1], n,
                     m // 4 - 1, sub, ctypes.c_float(alpha), ctypes.c_float(eps), loss.ctypes.data_as(F32),
                     grad.ctypes.data_as(F32))
    w, up = case['weight'].numpy(), case['up'].numpy()
    return torch.from_numpy(loss * w), torch.from_numpy(grad * (w * up)[:, None])


def check_rows_case(lib, kind, case, alpha, sub, what):
    ref, gref = lec.rows_statement(kind, case, alpha, torch.float64, sub=sub)
    assert torch.isfinite(ref).all() and torch.isfinite(gref).all(), what          # every row, none masked out
    assert lec.decisions_agree(case['pred'], case['target'], case['active'], alpha), what
    t32, g32 = lec.rows_statement(kind, case, alpha, torch.float32, sub=sub)
    got, ggot = host_rows(lib, kind, case, alpha, sub)
    judge(got, t32, ref, what + ' loss')
    lec.judge_rows(ggot, g32, gref, what + ' grad')
    dead = case['weight'] == 0
    assert dead.any() and not got[dead].any() and not ggot[dead].any(), what


@pytest.mark.parametrize('alpha', [0.25, 0.2])
@pytest.mark.parametrize('seed', [0, 1])
def test_bbox_edge_rows_through_the_host_compiled_row_function(rowlib, seed, alpha):  # noqa: F811
    case = lec.rows_case('bbox', seed, 2000, alpha=alpha)
    ties = lec.tie_counts(case['pred'], case['target'], case['active'], alpha)
    print(ties)
    assert ties['active'] > 100 and ties['pair'] > 100 and ties['pair_on_box'] > 50 and ties['negative'] > 1000
    assert (ties['inactive'] > 100) == (alpha == 0.25)
    # the planted box-edge ties are there: bx1 == gt[2] on every 7th row (object or not), and the three other edges
    p, an, gt = case['pred'], case['anchor'], case['gt']
    assert torch.equal((p[0::7, 15] + an[0::7, 0]), gt[0::7, 2]) and (p[0::7, 15] > p[0::7, 14]).all()
    assert torch.equal((-p[1::7, 0] + an[1::7, 1]), gt[1::7, 1]) and (p[1::7, 1] <= p[1::7, 0]).all()
    assert torch.equal((-p[2::7, 6] + an[2::7, 0]), gt[2::7, 0]) and torch.equal((p[3::7, 9] + an[3::7, 1]), gt[3::7, 3])
    check_rows_case(rowlib, 'bbox', case, alpha, 9, f'host bbox seed {seed} alpha {alpha}')


@pytest.mark.parametrize('alpha', [0.25, 0.2])
def test_stage_edge_rows_through_the_host_compiled_row_function(rowlib, alpha):  # noqa: F811
    case = lec.stage_case(5, 3000, alpha)
    what = f'host stage alpha {alpha}'
    ref, gref = lec.stage_statement(case, alpha)
    assert torch.isfinite(ref).all() and torch.isfinite(gref).all()
    target, active = lec.stage_targets(case, torch.float32)
    assert lec.decisions_agree(case['raw'], target, active, alpha)
    ties = lec.tie_counts(case['raw'], target, active, alpha)
    print(ties, int(case['on_anchor'].sum()))
    assert ties['active'] > 100 and ties['pair'] > 100 and ties['negative'] > 1000 and int(case['on_anchor'].sum()) > 1000
    t32, g32 = lec.stage_statement(case, alpha, torch.float32)
    n = len(case['raw'])
    loss, grad = np.zeros(n, np.float32), np.zeros((n, 20), np.float32)
    arrs = [_f(case[k]) for k in ('raw', 'gt_pts', 'anchor3', 'box')]
    obj = _u(case['weight'] > 0)
    rowlib.stage_rows(arrs[0][1], arrs[1][1], arrs[2][1], arrs[3][1], obj[1], n, ctypes.c_float(lec.BASE_SCALE),
                      ctypes.c_float(alpha), ctypes.c_float(1e-6), loss.ctypes.data_as(F32), grad.ctypes.data_as(F32))
    w, up = case['weight'].numpy(), case['up'].numpy()
    got, ggot = torch.from_numpy(loss * w), torch.from_numpy(grad * (w * up)[:, None])
    judge(got, t32, ref, what + ' loss')
    lec.judge_rows(ggot, g32, gref, what + ' grad')
    dead = case['weight'] == 0
    assert dead.sum() > 500 and not got[dead].any() and not ggot[dead].any()


POLY = [(36, 9), (9, 9), (36, 1), (36, 16)]
KEYPOINT_NV = [17, 4, 1]


@pytest.mark.parametrize('alpha', [0.25, 0.2])
@pytest.mark.parametrize('nv,sub', POLY)
def test_polygon_edge_rows_through_the_host_compiled_row_function(rowlib, nv, sub, alpha):  # noqa: F811
    case = lec.rows_case('polygon', 20 + nv + sub, 1500, nv, alpha)
    if nv == 36:
        assert lec.equal_extremes(case) >= 1                       # "first extreme wins" is exercised
    check_rows_case(rowlib, 'polygon', case, alpha, sub, f'host polygon nv {nv} sub {sub} alpha {alpha}')


@pytest.mark.parametrize('alpha', [0.25, 0.2])
@pytest.mark.parametrize('nv', KEYPOINT_NV)
def test_keypoint_edge_rows_through_the_host_compiled_row_function(rowlib, nv, alpha):  # noqa: F811
    case = lec.rows_case('keypoint', 40 + nv, 1500, nv, alpha)
    check_rows_case(rowlib, 'keypoint', case, alpha, 9, f'host keypoint nv {nv} alpha {alpha}')


# ------------------------------------------------------------------------------------------------------ the shape helper
def test_the_side_tensor_check_of_the_fused_rows():
    from lsnet_amd.ops import cross_iou as fused
    n = 6
    pred = torch.zeros(n, 20)
    good = ((torch.zeros(n, 20), (n, 20)), (torch.zeros(n, 20, dtype=torch.bool), (n, 20)), (torch.zeros(n, 2), (n, 2)),
            (torch.zeros(n, 4), (n, 4)), (None, (n,)), (torch.zeros(n), (n,)))
    assert fused.shapes_match(pred, good)
    for k in range(len(good)):
        if good[k][0] is None:
            continue
        for bad in (good[k][0][1:], good[k][0][..., None], good[k][0].reshape(-1)[:-1], good[k][0].to('meta')):
            if tuple(bad.shape) == good[k][1] and bad.device == pred.device:
                continue
            assert not fused.shapes_match(pred, good[:k] + ((bad, good[k][1]),) + good[k + 1:]), (k, bad.shape)
    # usable() hands every side tensor to it; on the CPU it is never usable, whatever the shapes
    assert not fused.usable(pred, good[0][0], 'bbox', good[1][0], good[2][0], good[3][0], good[5][0])
    # a mismatch reaches the torch formulation, which raises the ordinary shape error
    from lsnet_amd.models.losses import CrossIOULoss
    case = lec.rows_case('bbox', 0, n)
    with pytest.raises(RuntimeError):
        CrossIOULoss(loss_type='bbox')(case['pred'], case['target'], None, reduction_override='none',
                                       anchor_pts=case['anchor'][:-1], bbox_gt=case['gt'], pos_inds=case['active'])
