"""The corner-verification targets and losses as kernels of the library (csrc/cpv.hip) on the MI355X: through `hip_backend`,
the autograd functions of ops/cpv_loss.py and LSCPVHead, against the torch statements on the device (LSNET_NATIVE_CPV=0) and,
for the losses, both judged against a float64 evaluation of the same formulas (tests/cpv_cases.judge).  Inputs and their
near-tie condition: tests/cpv_cases.py."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lsnet_amd.core import PointHMAssigner
from lsnet_amd.models.losses import GaussianFocalLoss, SEPFocalLoss, SmoothL1Loss
from lsnet_amd.ops import cpv_loss
from tests import cpv_cases as cc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, GAMMA, BETA = 2.0, 4.0, 1.0 / 9.0


def _backend():
    from lsnet_amd.ops.backend import get_backend
    return get_backend(torch.zeros(1, device=DEV))


def _torch_statement(monkeypatch, fn, *args):
    with monkeypatch.context() as m:
        m.setattr(cpv_loss, 'NATIVE_CPV', False)
        return fn(*args)


# ---- 1. targets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cc.all_cases(), ids=lambda c: c[0])
def test_single_image_targets_equal_the_torch_statement(monkeypatch, case):
    name, hw, boxes = case
    pts, boxes = cc.grid(hw, DEV), boxes.to(DEV)
    for bump in (True, False):
        want = _torch_statement(monkeypatch, cc.statement, pts, None, boxes, bump)
        hm, off, npos = _backend().corner_targets_batch(pts, None, [boxes], bump, 0.7)
        cc.same_targets((hm[0], off[0], npos[0]), want, (name, bump))
        # the assigner's own interfaces go through the kernels too
        a = PointHMAssigner(bump, 0.7)
        got = a.assign_dense(pts, boxes, strides=cc.STRIDES)
        assert got[0].dtype == (torch.float32 if bump else torch.long)
        assert torch.equal(got[0].float(), hm[0, 0]) and torch.equal(got[1], off[0, 0])
        assert torch.equal(got[2].float(), hm[0, 1]) and torch.equal(got[3], off[0, 1])
        ref = _torch_statement(monkeypatch, a.assign, pts, boxes)
        for x, y in zip(a.assign(pts, boxes), ref):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x, y) if x.dtype == torch.long else bool(((x - y).abs() <= 5e-6 * y.abs()).all())


def test_batched_targets_equal_the_torch_statement(monkeypatch):
    """B = 3: the crowded image (seed 3: 134 positives of 200, shared cells), an image without gts, one with a valid mask"""
    pts = cc.grid(cc.GRID_A, DEV)
    P = len(pts)
    crowded = cc.boxes_of((cc.GRID_A, 3, 40)).to(DEV)
    masked = cc.boxes_of((cc.GRID_A, 5, 12)).to(DEV)
    mask = cc.valid_mask(P)
    assert cc.margins_ok(pts.cpu()[mask], masked.cpu())
    valid = torch.ones(3, P, dtype=torch.bool, device=DEV)
    valid[2] = mask.to(DEV)
    for bump in (True, False):
        hm, off, npos = _backend().corner_targets_batch(pts, valid, [crowded, crowded[:0], masked], bump, 0.7)
        cc.same_targets((hm[0], off[0], npos[0]), _torch_statement(monkeypatch, cc.statement, pts, None, crowded, bump), bump)
        assert not hm[1].any() and not off[1].any() and npos[1].tolist() == [0, 0]
        cc.same_targets((hm[2], off[2], npos[2]), _torch_statement(monkeypatch, cc.statement, pts, valid[2], masked, bump), bump)
    assert (npos[0] < 200).all() and (npos[0] > 100).all()            # 40 gts x 5 levels per corner, many cells shared
    # through the assigner, without a mask, into preallocated buffers
    a = PointHMAssigner(True, 0.7)
    hm2, off2, npos2 = a.assign_dense_batch(pts, None, [crowded, crowded[:0], masked])
    assert torch.equal(hm2[0], _backend().corner_targets_batch(pts, None, [crowded], True, 0.7)[0][0])
    lib_bytes = 64 + 52 * (2 * 16 * 4 + 8)
    out = (torch.empty_like(hm2), torch.empty_like(off2), torch.empty_like(npos2), torch.empty(lib_bytes, dtype=torch.uint8, device=DEV))
    _backend().corner_targets_batch(pts, None, [crowded, crowded[:0], masked], True, 0.7, out=out)
    assert torch.equal(out[0], hm2) and torch.equal(out[1], off2) and torch.equal(out[2], npos2)


def test_targets_equal_the_reference_fixture_on_the_device():
    """tests/golden/cpv_assigner.npz: the reference's own PointHMAssigner on 384 x 512 points, tolerance of tests/test_cpv.py"""
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'cpv_assigner.npz'))
    pts = cc.grid((384, 512), DEV)
    for seed, n in ((1, 5), (2, 9), (3, 1), (4, 30)):
        boxes = gu.make_gt(seed, n, 384, 512, num_classes=8)[0].to(DEV)
        for bump in (True, False):
            hm, off, npos = (t[0].cpu() for t in _backend().corner_targets_batch(pts, None, [boxes], bump, 0.7))
            for c, base in ((0, 0), (1, 4)):
                want_hm, want_off, want_pos = (torch.from_numpy(ref[f'{seed}/{int(bump)}/{base + i}']) for i in range(3))
                assert torch.allclose(hm[c], want_hm.float(), rtol=1e-6, atol=1e-7), (seed, bump, c)
                assert torch.allclose(off[c], want_off, rtol=1e-6, atol=1e-7), (seed, bump, c)
                assert torch.equal(torch.nonzero(hm[c] == 1).squeeze(-1), want_pos) and int(npos[c]) == len(want_pos)
    keep = torch.rand(pts.shape[0], generator=gu.gen(0)) < 0.7
    hm, off, _ = (t[0].cpu() for t in _backend().corner_targets_batch(pts, keep[None].to(DEV), [boxes], True, 0.7))
    for c, base in ((0, 0), (1, 4)):
        assert torch.allclose(hm[c][keep], torch.from_numpy(ref[f'keep/{base}']), rtol=1e-6, atol=1e-7)
        assert torch.allclose(off[c][keep], torch.from_numpy(ref[f'keep/{base + 1}']), rtol=1e-6, atol=1e-7)
        assert not hm[c][~keep].any() and not off[c][~keep].any()


# ---- 2. / 3. losses ---------------------------------------------------------------------------------------------------------
def statement_losses(scores, offsets, sems, hm, off, valid, npos, sem_map, sem_w, dtype):
    """The statements of LSCPVHead.loss (loss weights 1) in `dtype` on the tensors' device -> (heat (L,), offs (L,), sem)"""
    def c(t):
        return t.to(dtype)
    loss_heatmap, loss_offset, loss_sem = GaussianFocalLoss(ALPHA, GAMMA), SmoothL1Loss(BETA), SEPFocalLoss(2.0, 0.25)
    num_level = [s.shape[2] * s.shape[3] for s in scores]
    live = torch.ones_like(hm[:, 0]) if valid is None else valid.to(hm.dtype)
    n = npos.clamp(min=1).sum(0)
    heat, offs = [], []
    for lvl in range(len(scores)):
        score = c(scores[lvl]).permute(0, 2, 3, 1).reshape(-1, 2).sigmoid()
        o = c(offsets[lvl]).permute(0, 2, 3, 1).reshape(-1, 4)
        lh = lo = 0
        for col in (0, 1):
            t = torch.split(hm[:, col], num_level, dim=1)[lvl].reshape(-1)
            w = torch.split(live, num_level, dim=1)[lvl].reshape(-1)
            ot = torch.split(off[:, col], num_level, dim=1)[lvl].reshape(-1, 2)
            ow = ((t == 1).to(dtype) * c(w)).unsqueeze(1).expand(-1, 2)
            lh = lh + loss_heatmap(score[:, col], c(t), c(w), avg_factor=n[col])
            lo = lo + loss_offset(o[:, 2 * col:2 * col + 2], c(ot), ow, avg_factor=n[col])
        heat.append(lh / 2.0)
        offs.append(lo / 2.0)
    sem_pred = torch.cat([c(s).reshape(-1) for s in sems])
    sem_gt = torch.cat([F.interpolate(sem_map, s.shape[-2:]).reshape(-1) for s in sems])
    sem_wt = torch.cat([F.interpolate(sem_w, s.shape[-2:]).reshape(-1) for s in sems])
    return torch.stack(heat), torch.stack(offs), loss_sem(sem_pred, c(sem_gt), c(sem_wt), avg_factor=(sem_gt > 0).sum())


def _loss_case(levels, channels_last, seed=0, B=2, C=3):
    """random maps over the given levels of the 264 x 376 grid, targets from the kernels: the crowded image and the large
    boxes (46 / 30 bump points), the second image under a valid mask"""
    sizes = cc.level_sizes(cc.GRID_A)
    pts = torch.cat([p for p, s in zip(torch.split(cc.grid(cc.GRID_A), [h * w for h, w in sizes]), sizes) if s in levels]).to(DEV)
    g = gu.gen(100 + seed)
    fmt = torch.channels_last if channels_last else torch.contiguous_format

    def maps(ch, scale, shift=0.0):
        return [(torch.randn(B, ch, h, w, generator=g) * scale + shift).to(DEV).contiguous(memory_format=fmt) for h, w in levels]
    scores, offsets, sems = maps(2, 1.5, -1.0), maps(4, 0.3), maps(C, 1.5, -1.0)
    valid = torch.ones(B, len(pts), dtype=torch.bool, device=DEV)
    valid[1] = cc.valid_mask(len(pts), seed=3).to(DEV)
    boxes = [cc.boxes_of((cc.GRID_A, 3, 40)).to(DEV), torch.tensor(cc.LARGE_BOXES, device=DEV)]
    hm, off, npos = _backend().corner_targets_batch(pts, valid, boxes, True, 0.7)
    h8, w8 = sizes[0]
    sem_map = (torch.rand(B, C, h8, w8, generator=g) > 0.8).float()
    sem_map[:, :, ::5, ::7] = 0.5                                  # counted by target > 0, a negative of the loss
    sem_w = torch.rand(B, C, h8, w8, generator=g) + 0.1
    return scores, offsets, sems, hm, off, valid, npos, sem_map.to(DEV), sem_w.to(DEV)


def _arms(case):
    """-> {arm: (values (heat, offs, sem), gradients of their sum w.r.t. every map)} for 'native', 'torch' (fp32 statement on
    the device) and 'ref' (the statement in float64)"""
    scores, offsets, sems, hm, off, valid, npos, sem_map, sem_w = case
    out = {}
    for arm in ('native', 'torch', 'ref'):
        dt = torch.float64 if arm == 'ref' else torch.float32
        leaves = [t.detach().to(dt).clone(memory_format=torch.preserve_format).requires_grad_() for t in scores + offsets + sems]
        L = len(scores)
        s, o, m = leaves[:L], leaves[L:2 * L], leaves[2 * L:]
        if arm == 'native':
            heat, offs = cpv_loss.corner_losses(s, o, hm, off, valid, npos, ALPHA, GAMMA, BETA)
            sem = cpv_loss.sep_focal_loss(m, sem_map, sem_w, 2.0, 0.25)
        else:
            heat, offs, sem = statement_losses(s, o, m, hm, off, valid, npos, sem_map, sem_w,
                                               torch.float32 if arm == 'torch' else torch.float64)
        # distinct upstream gradients per level and loss, so that a swapped level shows
        k = torch.arange(1, L + 1, device=DEV, dtype=heat.dtype)
        ((heat * k).sum() + (offs * (k + 0.5)).sum() + 3.0 * sem).backward()
        out[arm] = ((heat.detach(), offs.detach(), sem.detach()), [t.grad for t in leaves])
    return out


LEVEL_LISTS = {'three': [(9, 12), (5, 6), (3, 3)], 'five': cc.level_sizes(cc.GRID_A)}


@pytest.mark.parametrize('channels_last', [False, True], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('levels', ['three', 'five'])
def test_losses_against_the_torch_statement(levels, channels_last):
    arms = _arms(_loss_case(LEVEL_LISTS[levels], channels_last))
    names = ('loss_heatmap', 'loss_offset', 'loss_sem')
    for i, name in enumerate(names):
        n, t, r = (arms[a][0][i].reshape(-1) for a in ('native', 'torch', 'ref'))
        for l in range(n.numel()):
            cc.judge(n[l], t[l], r[l], f'{levels} {name}[{l}]')
    L = len(LEVEL_LISTS[levels])
    for j, (n, t, r) in enumerate(zip(*(arms[a][1] for a in ('native', 'torch', 'ref')))):
        assert n.shape == r.shape and torch.isfinite(n).all()
        cc.judge(n, t, r, f'{levels} gradient of {("score", "offset", "sem")[j // L]} map {j % L}')


def test_losses_are_bit_reproducible():
    case = _loss_case(LEVEL_LISTS['five'], False)
    a, b = _arms(case)['native'], _arms(case)['native']
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    pts = cc.grid(cc.GRID_A, DEV)
    boxes = [cc.boxes_of((cc.GRID_A, 3, 40)).to(DEV)]
    t1, t2 = (_backend().corner_targets_batch(pts, None, boxes, True, 0.7) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(t1, t2))


def test_semantic_loss_without_positives_is_the_statements(monkeypatch):
    """no target == 1: the positive term is 0; count(target > 0) > 0 through the 0.5 cells"""
    scores, offsets, sems, hm, off, valid, npos, sem_map, sem_w = _loss_case(LEVEL_LISTS['three'], False)
    sem_map = torch.where(sem_map == 1, torch.zeros_like(sem_map), sem_map)
    got = cpv_loss.sep_focal_loss(sems, sem_map, sem_w, 2.0, 0.25)
    want = statement_losses(scores, offsets, sems, hm, off, valid, npos, sem_map, sem_w, torch.float64)[2]
    assert torch.isfinite(got) and abs(float(got) - float(want)) <= 1e-6 * abs(float(want))


# ---- 4. the head --------------------------------------------------------------------------------------------------------------
def _head():
    from lsnet_amd.models import build_head
    from lsnet_amd.utils import ConfigDict
    cfg, tr, te = gu.cpv_head_cfg()
    mc = ConfigDict(copy.deepcopy(cfg))
    mc.update(train_cfg=ConfigDict(tr), test_cfg=ConfigDict(te))
    return gu.fill_params(build_head(mc), seed=7).to(DEV).train()


CPV_KEYS = ('loss_heatmap', 'loss_offset', 'loss_sem')


def test_head_loss_and_backward_native_against_the_switch(monkeypatch):
    from tests import golden_cases as gc
    head = _head()
    with torch.no_grad():
        outs = head([f.to(DEV) for f in gu.head_inputs(11)])
    boxes, labels, extremes, _, _, metas = gc.gt_for('bbox', DEV)
    sem, wts = gu.make_sem_maps([b.cpu() for b in boxes], [l.cpu() for l in labels], *gu.HEAD_IMG, 8)
    sem, wts = sem.to(DEV), wts.to(DEV)

    def run(native):
        leaves = [[t.detach().clone().requires_grad_() for t in lv] for lv in outs]
        fn = lambda: head.loss(*leaves, boxes, extremes, sem, wts, labels, metas)      # noqa: E731
        losses = fn() if native else _torch_statement(monkeypatch, fn)
        sum(sum(losses[k]) if isinstance(losses[k], list) else losses[k] for k in CPV_KEYS).backward()
        return losses, [t.grad for lv in leaves[3:] for t in lv]
    got, g_got = run(True)
    want, g_want = run(False)
    assert sorted(got) == sorted(want)
    for k in got:
        assert isinstance(got[k], list) == isinstance(want[k], list) and (not isinstance(got[k], list) or len(got[k]) == len(want[k]))
        if k not in CPV_KEYS:                                       # LSHead's part is the same code in both arms
            a, b = torch.stack(list(got[k])) if isinstance(got[k], list) else got[k], \
                torch.stack(list(want[k])) if isinstance(want[k], list) else want[k]
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-7), k
    # the float64 evaluation of the statements on the torch arm's own targets
    points, flags, all_valid = head.get_points([tuple(m.shape[-2:]) for m in outs[0]], metas, torch.device(DEV))
    tg = _torch_statement(monkeypatch, head.get_hm_targets, torch.cat(points), [torch.cat(f) for f in flags], all_valid, boxes)[0]
    hm = torch.stack([tg['hm_tl'], tg['hm_br']], 1)
    off = torch.stack([tg['off_tl'], tg['off_br']], 1)
    npos = (hm == 1).sum(2).int()
    leaves = [[t.detach().double().requires_grad_() for t in lv] for lv in outs[3:]]
    heat, offs, sl = statement_losses(*leaves, hm, off, None, npos, sem, wts, torch.float64)
    lw = (head.loss_heatmap.loss_weight, head.loss_offset.loss_weight, head.loss_sem.loss_weight)
    (lw[0] * heat.sum() + lw[1] * offs.sum() + lw[2] * sl).backward()
    ref = dict(loss_heatmap=lw[0] * heat, loss_offset=lw[1] * offs, loss_sem=(lw[2] * sl).reshape(1))
    for k in CPV_KEYS:
        n, t = (torch.stack(list(d[k])) if isinstance(d[k], list) else d[k].reshape(1) for d in (got, want))
        for l in range(n.numel()):
            cc.judge(n[l], t[l], ref[k][l], f'head {k}[{l}]')
    for j, (n, t, r) in enumerate(zip(g_got, g_want, [t.grad for lv in leaves for t in lv])):
        cc.judge(n, t, r, f'head gradient {j}')


@pytest.mark.parametrize('case', ['empty', 'ragged'])
def test_head_edge_cases_equal_the_reference(case):
    """an image without objects / an image smaller than the padded batch (valid mask), tests/golden/edge_targets.npz at
    that fixture's own rtol"""
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'edge_targets.npz'))
    head = _head()
    boxes, labels, ext, metas, sem, wts = gu.edge_case_targets(case)
    boxes, labels, ext = ([t.to(DEV) for t in lst] for lst in (boxes, labels, ext))
    outs = head([f.to(DEV) for f in gu.head_inputs(11)])
    losses = head.loss(*outs, boxes, ext, sem.to(DEV), wts.to(DEV), labels, metas)
    tag = f'cpv/{case}/'
    want = {k[len(tag):]: ref[k] for k in ref if k.startswith(tag)}
    got = {k: np.array([float(x) for x in (v if isinstance(v, (list, tuple)) else [v])]) for k, v in losses.items()}
    assert sorted(want) == sorted(got)
    for k in want:
        assert np.allclose(want[k], got[k], rtol=1e-4, atol=1e-6), (k, want[k], got[k])
        assert np.isfinite(got[k]).all()


def test_native_calls_read_nothing_back():
    """targets, losses and their backward under torch's synchronisation check: no device -> host read, no blocking copy"""
    head = _head()
    boxes, labels, ext, metas, sem, wts = gu.edge_case_targets('ragged')
    boxes = [b.to(DEV) for b in boxes]
    sem, wts = sem.to(DEV), wts.to(DEV)
    with torch.no_grad():
        outs = head([f.to(DEV) for f in gu.head_inputs(11)])
    hm_scores, hm_offsets, sem_scores = ([t.detach().clone().requires_grad_() for t in lv] for lv in outs[3:])
    points, flags, all_valid = head.get_points([tuple(m.shape[-2:]) for m in outs[0]], metas, torch.device(DEV))
    flat_points, flat_flags = torch.cat(points), [torch.cat(f) for f in flags]
    assert not all_valid
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        hm, off, valid, npos = head.get_hm_targets_native(flat_points, flat_flags, all_valid, boxes)
        heat, offs = cpv_loss.corner_losses(hm_scores, hm_offsets, hm, off, valid, npos, ALPHA, GAMMA, BETA)
        sl = cpv_loss.sep_focal_loss(sem_scores, sem, wts, 2.0, 0.25)
        (heat.sum() + offs.sum() + sl).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert valid is not None and all(t.grad is not None for t in hm_scores + hm_offsets + sem_scores)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_text_and_launch_nothing():
    from lsnet_amd import _lib
    be = _backend()
    pts = cc.grid(cc.GRID_B, DEV)
    P = len(pts)
    boxes = cc.boxes_of((cc.GRID_B, 7, 5)).to(DEV)

    def sentinel(B):
        return (torch.full((B, 2, P), 7.0, device=DEV), torch.full((B, 2, P, 2), 7.0, device=DEV),
                torch.full((B, 2), 7, dtype=torch.int32, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV))
    out = sentinel(65)
    with pytest.raises(RuntimeError, match='65 images'):
        be.corner_targets_batch(pts, None, [boxes] * 65, True, 0.7, out=out)
    assert b'65 images' in _lib.load().lsn_last_error()
    assert (out[0] == 7).all() and (out[1] == 7).all() and (out[2] == 7).all()
    with pytest.raises(RuntimeError, match='P = 0'):
        be.corner_targets_batch(pts[:0], None, [boxes], True, 0.7)
    with pytest.raises(TypeError, match='float32'):
        be.corner_targets_batch(pts.double(), None, [boxes], True, 0.7)
    with pytest.raises(TypeError, match='float32'):
        be.corner_targets_batch(pts, None, [boxes.half()], True, 0.7)
    assert PointHMAssigner(True, 0.7).assign_dense_batch(pts.double(), None, [boxes.double()]) is None    # the torch path's
    # more than 8 levels
    hm, off, npos = be.corner_targets_batch(pts[:9], None, [boxes], True, 0.7)
    scores = [torch.zeros(1, 2, 1, 1, device=DEV) for _ in range(9)]
    offsets = [torch.zeros(1, 4, 1, 1, device=DEV) for _ in range(9)]
    heat, offl = torch.full((9,), 7.0, device=DEV), torch.full((9,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match='9 levels'):
        be.corner_loss_forward(scores, offsets, hm, off, None, npos, ALPHA, GAMMA, BETA,
                               out=(heat, offl, torch.zeros(64, dtype=torch.float64, device=DEV)))
    assert b'9 levels' in _lib.load().lsn_last_error() and (heat == 7).all() and (offl == 7).all()
    sems = [torch.zeros(1, 3, 1, 1, device=DEV) for _ in range(9)]
    with pytest.raises(RuntimeError, match='9 levels'):
        be.sep_focal_forward(sems, torch.zeros(1, 3, 2, 2, device=DEV), torch.zeros(1, 3, 2, 2, device=DEV), 2.0, 0.25)
    with pytest.raises(TypeError, match='float32'):
        be.sep_focal_forward(sems[:2], torch.zeros(1, 3, 2, 2, device=DEV).double(), torch.zeros(1, 3, 2, 2, device=DEV), 2.0, 0.25)
    # levels that do not add up to the targets' points
    with pytest.raises(ValueError, match='points'):
        be.corner_loss_forward(scores[:8], offsets[:8], hm, off, None, npos, ALPHA, GAMMA, BETA)
