"""LSHead's point decoding as library kernels (csrc/points.hip) against the torch statements they replace, on the device.

Through the C ABI and the ops (ops/point_decode.py): for every layout of tests/point_decode_cases.py, forward and backward of
point_decode, softplus_add and point_boxes.  sp, the softplus derivative and softplus_add are compared with ATen's device
results; everything behind the softplus -- off, the scatter into g_raw, the free channels, the boxes -- with the torch statements
applied to the kernel's own sp.  All comparisons are torch.equal: SOFTPLUS_BIT_EQUAL below records that the kernels' softplus
and derivative are ATen's bit for bit on the MI355X (the same expf / log1pf of the device math library), so nothing is
loosened anywhere, and the head with the switch on and off agrees bit for bit as well.  Measured there against float64, kernel
and ATen alike: softplus 1.55 ulp, derivative 2.29 ulp, softplus_add 1.43 ulp at worst over the cases (the tests print them),
inside the derived bound of 4 ulp.

Through the head: a small LSHead (32 channels, 4 GN groups, seeded init_weights, levels 7x11 / 4x6 / 2x3, B = 2) for the tasks
bbox, segm, pose_bbox and pose_kbox with NATIVE_POINTS on and off: the 7-tuple of forward, the proposal boxes of
refine_stage_targets, the refine-stage gt_inds for three ground-truth boxes per image and every parameter gradient of a
seeded linear functional of all outputs.

Launches: the library's event log counts one point_decode and one softplus_add launch per branch and forward, the same again
in backward, and one point_boxes launch per refine_stage_targets."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import golden_util as gu
from tests import point_decode_cases as pc

pytestmark = pytest.mark.gpu
SOFTPLUS_BIT_EQUAL = True      # kernel softplus / derivative == ATen's on the device, bit for bit (asserted below)
ULP_BOUND = 4.0                # tests/test_point_decode_host.py derives it


def _dev():
    return torch.device('cuda:0')


_DEV_CASES = {}


def _case(name):
    """the shared case on the device (copied once, never written to) with its table and base grid"""
    from lsnet_amd.ops.point_decode import offset_sources
    if name not in _DEV_CASES:
        c = dict(pc.case(name))
        for k in ('raw', 'g_sp', 'g_off', 'res', 'g_ref'):
            c[k] = c[k].to(_dev())
        c['src'] = offset_sources(c['task'], c['n_sp'], c['c_raw'], 9)
        c['base64'] = pc.base_offset().to(_dev())
        c['base'] = c['base64'].float()
        c['points'] = pc.flat_points().to(_dev())
        _DEV_CASES[name] = c
    return _DEV_CASES[name]


def _leaf(rows):
    return pc.px(rows.clone()).requires_grad_()


def _decode(c, raw4):
    from lsnet_amd.ops.point_decode import point_decode
    return point_decode(raw4, c['n_sp'], c['src'], pc.GM, c['base'])


def _reference(c, sp_kernel, raw4, g_sp4, g_off4):
    """The torch statements from the kernel's own sp on: (off, the gradient that reaches sp, the gradient of the free
    channels or None); either output gradient may be None."""
    sp_in = sp_kernel.detach().clone().requires_grad_()
    raw_in = raw4.detach().clone().requires_grad_()
    off = pc.offsets_from_sp(c, sp_in, raw_in, base=c['base64'])
    outs, grads = [], []
    if g_off4 is not None:
        outs.append(off), grads.append(g_off4)
    if g_sp4 is not None:
        outs.append(sp_in * 1.0), grads.append(g_sp4)
    g_pre, g_rawin = torch.autograd.grad(outs, [sp_in, raw_in], grads, allow_unused=True)
    g_free = None if g_rawin is None else g_rawin[:, c['n_sp']:]
    return off.detach(), g_pre, g_free


def _ulp_report(what, got, aten, ref64):
    k, a = pc.ulp_error(got, ref64).max().item(), pc.ulp_error(aten, ref64).max().item()
    print(f'POINTS {what}: kernel {k:.2f} ulp, ATen {a:.2f} ulp against float64; bit-equal {torch.equal(got, aten)}')
    return k, a


# ---- the ops against the torch statements ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(pc.LAYOUTS))
def test_point_decode_forward_and_backward(name):
    c = _case(name)
    n_sp = c['n_sp']
    raw4 = _leaf(c['raw'])
    sp, off = _decode(c, raw4)
    assert tuple(sp.shape) == (pc.B, n_sp, pc.N_ALL, 1) and tuple(off.shape) == (pc.B, 18, pc.N_ALL, 1)
    assert sp.stride(1) == 1 and off.stride(1) == 1 and sp.stride(2) == n_sp and off.stride(2) == 18
    g_sp4, g_off4 = pc.px(c['g_sp']), pc.px(c['g_off'])
    g_raw, = torch.autograd.grad([sp, off], raw4, [g_sp4, g_off4])
    ones, = torch.autograd.grad([_decode(c, raw4)[0]], raw4, [torch.ones_like(sp)])         # the derivative factor alone
    torch.cuda.synchronize()

    # softplus and its derivative: ATen's bits (and within the derived bound of float64)
    x = raw4.detach()[:, :n_sp]
    sp_aten = F.softplus(x)
    d_aten = torch.ops.aten.softplus_backward(torch.ones_like(x), x, 1.0, 20.0)
    k, a = _ulp_report(f'{name} softplus', sp.detach(), sp_aten, pc.softplus64(x))
    kd, ad = _ulp_report(f'{name} derivative', ones[:, :n_sp], d_aten, pc.softplus_grad64(x))
    assert k <= ULP_BOUND and kd <= ULP_BOUND and k <= a + 1 and kd <= ad + 1
    assert torch.equal(sp.detach(), sp_aten) and torch.equal(ones[:, :n_sp], d_aten)
    assert not ones[:, n_sp:].any()

    # behind the softplus: the torch statements on the kernel's own sp
    off_ref, g_pre, g_free = _reference(c, sp, raw4, g_sp4, g_off4)
    assert torch.equal(off.detach(), off_ref)
    assert torch.equal(g_raw[:, :n_sp], torch.ops.aten.softplus_backward(g_pre, x, 1.0, 20.0))
    if c['c_raw'] > n_sp:
        assert torch.equal(g_raw[:, n_sp:], g_free)
    # a tie gives -neg and sends its gradient to neg, negated: row 0 is all ties, and channel 0 of off reads the pair src[0]
    j0 = c['src'][0]
    gm_g = torch.tensor(pc.GM, dtype=torch.float32, device=_dev()) * c['g_off'][0, 0, 0]
    scatter = _reference(c, sp, raw4, None, g_off4)[1]
    assert torch.equal(scatter[0, j0:j0 + 2, 0, 0], torch.stack([-gm_g, gm_g * 0]))
    assert torch.equal(sp[0, j0, 0, 0], sp[0, j0 + 1, 0, 0])
    # and the whole thing is what autograd makes of the head's statements from raw on
    raw_t = raw4.detach().clone().requires_grad_()
    sp_t, off_t = pc.head_statements(c, raw_t, base=c['base64'])
    g_t, = torch.autograd.grad([sp_t, off_t], raw_t, [g_sp4, g_off4])
    assert torch.equal(sp.detach(), sp_t.detach()) and torch.equal(off.detach(), off_t.detach()) and torch.equal(g_raw, g_t)


@pytest.mark.parametrize('name', ['bbox', 'segm', 'pose'])
def test_point_decode_partial_requests(name):
    from lsnet_amd import _lib
    c = _case(name)
    n_sp = c['n_sp']
    raw4 = _leaf(c['raw'])
    x = raw4.detach()[:, :n_sp]
    g_sp4, g_off4 = pc.px(c['g_sp']), pc.px(c['g_off'])
    for gs, go in ((None, g_off4), (g_sp4, None)):
        sp, off = _decode(c, raw4)
        outs, grads = ([off], [go]) if gs is None else ([sp], [gs])
        g_raw, = torch.autograd.grad(outs, raw4, grads)
        _, g_pre, g_free = _reference(c, sp, raw4, gs, go)
        assert torch.equal(g_raw[:, :n_sp], torch.ops.aten.softplus_backward(g_pre, x, 1.0, 20.0))
        if c['c_raw'] > n_sp:
            assert torch.equal(g_raw[:, n_sp:], torch.zeros_like(g_raw[:, n_sp:]) if g_free is None or go is None else g_free)
    # a raw that needs no gradient: outputs without history, one launch in all
    try:
        _lib.prof_enable(True, ['points'])
        sp, off = _decode(c, raw4.detach())
        torch.cuda.synchronize()
        log = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    assert not sp.requires_grad and not off.requires_grad and log['points']['launches'] == 1


@pytest.mark.parametrize('name', sorted(pc.LAYOUTS))
def test_softplus_add(name):
    from lsnet_amd.ops.point_decode import softplus_add
    c = _case(name)
    sp = _decode(c, pc.px(c['raw']))[0]
    a = _leaf(c['res'])
    y = softplus_add(a, sp)
    ga, = torch.autograd.grad(y, a, pc.px(c['g_ref']))
    a_t = a.detach().clone().requires_grad_()
    y_t = torch.nn.Softplus()(a_t + sp.detach())
    ga_t, = torch.autograd.grad(y_t, a_t, pc.px(c['g_ref']))
    k, at = _ulp_report(f'{name} softplus_add', y.detach(), y_t.detach(), pc.softplus64(a.detach() + sp))
    assert k <= ULP_BOUND and k <= at + 1
    assert tuple(y.shape) == tuple(a.shape) and y.stride(1) == 1
    assert torch.equal(y.detach(), y_t.detach()) and torch.equal(ga, ga_t)
    assert not softplus_add(a.detach(), sp).requires_grad


@pytest.mark.parametrize('name', sorted(pc.LAYOUTS))
def test_point_boxes(name):
    from lsnet_amd.ops.point_decode import point_boxes
    c = _case(name)
    sp = _decode(c, pc.px(c['raw']))[0]
    mode, nv = pc.box_mode(c)
    got = point_boxes(pc.rows_of(sp), c['points'], mode, nv)
    want = pc.boxes_from_sp(c, sp, c['points'])
    assert tuple(got.shape) == (pc.B, pc.N_ALL, 4) and torch.equal(got, want)
    if mode == 'vectors':       # fewer vectors than lanes per row, and a count that is no multiple of them
        for n in (1, 5, 16, 17):
            c2 = dict(c, nv=n)
            assert torch.equal(point_boxes(pc.rows_of(sp), c['points'], mode, n),
                               pc.boxes_from_sp(c2, sp[:, :4 * n + 4], c['points']))


# ---- pitches and alignments: the 16-byte path only where pointer and pitch allow it -------------------------------------------
@pytest.mark.parametrize('name', ['bbox', 'segm'])
@pytest.mark.parametrize('lead,extra', [(3, 5), (4, 8)])      # an unaligned column slice; an aligned one with a wider pitch
def test_pitched_rows_through_the_c_abi(name, lead, extra):
    from lsnet_amd import _lib
    from lsnet_amd.ops.hip_backend import HipBackend
    lib = _lib.load()
    c = _case(name)
    n_sp, c_raw, R = c['n_sp'], c['c_raw'], pc.B * pc.N_ALL
    raw4 = _leaf(c['raw'])
    sp_d, off_d = _decode(c, raw4)
    g_d, = torch.autograd.grad([sp_d, off_d], raw4, [pc.px(c['g_sp']), pc.px(c['g_off'])])
    nan = float('nan')
    wide = torch.full((R, c_raw + extra), nan, device=_dev())
    wide[:, lead:lead + c_raw] = c['raw'].reshape(R, c_raw)
    raw = wide[:, lead:lead + c_raw]
    off = torch.full((R, 20), nan, device=_dev())
    sp = torch.full((R, n_sp + extra), nan, device=_dev())
    table = HipBackend._point_table(c['src'])
    rc = lib.lsn_point_decode_forward(raw.data_ptr(), wide.stride(0), c_raw, n_sp, table, 18, pc.GM, c['base'].data_ptr(),
                                      sp[:, lead:].data_ptr(), sp.stride(0), off.data_ptr(), 20, R, _lib.stream())
    assert rc == 0, lib.lsn_last_error()
    g_sp = torch.full((R, n_sp + extra), nan, device=_dev())
    g_sp[:, lead:lead + n_sp] = c['g_sp'].reshape(R, n_sp)
    g_off = torch.full((R, 20), nan, device=_dev())
    g_off[:, :18] = c['g_off'].reshape(R, 18)
    g_raw = torch.full((R, c_raw + extra), nan, device=_dev())
    rc = lib.lsn_point_decode_backward(raw.data_ptr(), wide.stride(0), c_raw, n_sp, table, 18, pc.GM, sp[:, lead:].data_ptr(),
                                       sp.stride(0), g_sp[:, lead:].data_ptr(), g_sp.stride(0), g_off.data_ptr(), 20,
                                       g_raw[:, lead:].data_ptr(), g_raw.stride(0), R, _lib.stream())
    assert rc == 0, lib.lsn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(sp[:, lead:lead + n_sp], pc.rows_of(sp_d.detach()).reshape(R, n_sp))
    assert torch.equal(off[:, :18], pc.rows_of(off_d.detach()).reshape(R, 18))
    assert torch.equal(g_raw[:, lead:lead + c_raw], pc.rows_of(g_d).reshape(R, c_raw))
    # nothing beside the rows was written
    assert torch.isnan(off[:, 18:]).all() and torch.isnan(sp[:, :lead]).all() and torch.isnan(sp[:, lead + n_sp:]).all()
    assert torch.isnan(g_raw[:, :lead]).all() and torch.isnan(g_raw[:, lead + c_raw:]).all()


@pytest.mark.parametrize('lead', [1, 4])
def test_sliced_rows_through_the_ops(lead):
    """softplus_add and point_boxes on column slices of wider buffers (lead 1: unaligned, one float per lane)"""
    from lsnet_amd.ops.point_decode import point_boxes, softplus_add
    c = _case('segm')
    n_sp = c['n_sp']
    sp = _decode(c, pc.px(c['raw']))[0]
    buf = torch.zeros(pc.B, pc.N_ALL, n_sp + 8, device=_dev())
    buf[:, :, lead:lead + n_sp] = pc.rows_of(sp)
    rows = buf[:, :, lead:lead + n_sp]
    assert torch.equal(point_boxes(rows, c['points'], 'vectors', c['nv']), pc.boxes_from_sp(c, sp, c['points']))
    abuf = torch.zeros(pc.B, pc.N_ALL, n_sp + 8, device=_dev())
    abuf[:, :, lead:lead + n_sp] = c['res']
    a = abuf[:, :, lead:lead + n_sp].requires_grad_()
    y = softplus_add(a, rows)
    ga, = torch.autograd.grad(y, a, c['g_ref'])
    a_t = c['res'].clone().requires_grad_()
    y_t = F.softplus(a_t + pc.rows_of(sp))
    ga_t, = torch.autograd.grad(y_t, a_t, c['g_ref'])
    assert torch.equal(y.detach(), y_t.detach()) and torch.equal(ga, ga_t)


def test_argument_errors_are_refused_before_any_launch():
    from lsnet_amd import _lib
    from lsnet_amd.ops.hip_backend import HipBackend
    lib = _lib.load()
    c = _case('bbox')
    R = pc.B * pc.N_ALL
    raw = c['raw'].reshape(R, 28)
    sp, off = torch.full((R, 20), 7.0, device=_dev()), torch.full((R, 18), 7.0, device=_dev())
    good = HipBackend._point_table(c['src'])

    def fwd(raw_p=raw.data_ptr(), pitch=28, n_sp=20, table=good, base=c['base'].data_ptr(), sp_p=sp.data_ptr(), off_pitch=18):
        return lib.lsn_point_decode_forward(raw_p, pitch, 28, n_sp, table, 18, pc.GM, base, sp_p, 20, off.data_ptr(), off_pitch, R,
                                            _lib.stream())
    outside = (ctypes.c_int * 18)(*((20,) + c['src'][1:]))
    free_out = (ctypes.c_int * 18)(*(c['src'][:17] + (-9,)))
    twice = (ctypes.c_int * 18)(*((c['src'][1],) + c['src'][1:]))
    for what, rc in (('NULL raw', fwd(raw_p=None)), ('NULL base', fwd(base=None)), ('NULL sp', fwd(sp_p=None)),
                     ('NULL table', fwd(table=None)), ('n_sp 18', fwd(n_sp=18)), ('pick outside', fwd(table=outside)),
                     ('free outside', fwd(table=free_out)), ('pick twice', fwd(table=twice)), ('raw pitch', fwd(pitch=27)),
                     ('off pitch', fwd(off_pitch=17))):
        assert rc == -1 and lib.lsn_last_error(), what
    a = c['res'].reshape(R, 20)
    assert lib.lsn_softplus_add_forward(a.data_ptr(), 20, None, 20, sp.data_ptr(), 20, 20, R, _lib.stream()) == -1
    assert lib.lsn_softplus_add_backward(a.data_ptr(), 20, a.data_ptr(), 19, a.data_ptr(), 20, sp.data_ptr(), 20, 20, R,
                                         _lib.stream()) == -1
    box = torch.full((R, 4), 7.0, device=_dev())
    for args in ((None, 20, 20, c['points'].data_ptr(), pc.N_ALL, pc.B, 0, 4), (a.data_ptr(), 20, 20, None, pc.N_ALL, pc.B, 0, 4),
                 (a.data_ptr(), 20, 20, c['points'].data_ptr(), pc.N_ALL, pc.B, 2, 4),
                 (a.data_ptr(), 20, 20, c['points'].data_ptr(), pc.N_ALL, pc.B, 1, 6),
                 (a.data_ptr(), 12, 12, c['points'].data_ptr(), pc.N_ALL, pc.B, 0, 4)):
        assert lib.lsn_point_boxes(*args, box.data_ptr(), 4, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert (sp == 7).all() and (off == 7).all() and (box == 7).all()


# ---- through the head ----------------------------------------------------------------------------------------------------------
HEAD_IMG = (56, 88)       # -> the levels of point_decode_cases at strides 8, 16, 32
TASKS = ['bbox', 'segm', 'pose_bbox', 'pose_kbox']


def _head(task):
    from lsnet_amd.models import build_head
    from lsnet_amd.utils import ConfigDict
    cfg, train_cfg, test_cfg = gu.head_cfg(task, 32)
    cfg = copy.deepcopy(cfg)
    cfg['norm_cfg'] = dict(type='GN', num_groups=4, requires_grad=True)
    cfg['point_strides'] = list(pc.STRIDES)
    cfg = ConfigDict(cfg)
    train_cfg = copy.deepcopy(train_cfg)
    train_cfg['refine']['assigner']['topk'] = 5          # (the 2x3 level has 6 cells: ATSS takes no level shorter than topk)
    cfg.update(train_cfg=ConfigDict(train_cfg), test_cfg=ConfigDict(test_cfg))
    head = build_head(cfg)
    torch.manual_seed(5)
    head.init_weights()
    return head.to(_dev()).train()


def _head_inputs(task):
    g = pc.gen(77)
    feats = [torch.randn(pc.B, 32, h, w, generator=g).to(_dev()).contiguous(memory_format=torch.channels_last)
             for h, w in pc.LEVELS]
    h, w = HEAD_IMG
    boxes, labels, extremes, masks, kps = [], [], [], [], []
    for i in range(pc.B):
        b, l, e = gu.make_gt(300 + i, 3, h, w, num_classes=8, min_size=8.)
        boxes.append(b.to(_dev())), labels.append(l.to(_dev())), extremes.append(e.to(_dev()))
        masks.append(gu.make_polygons(b))
        kps.append(gu.make_keypoints(400 + i, b).to(_dev()))
    metas = [dict(pad_shape=(h, w, 3), img_shape=(h, w, 3), scale_factor=1.0) for _ in range(pc.B)]
    gt = (boxes, extremes if task in ('bbox', 'pose_bbox') else None, [k.clone() for k in kps] if 'pose' in task else None,
          masks if task == 'segm' else None, labels, metas)
    return feats, gt


def _run_head(head, feats, gt, native, monkeypatch):
    from lsnet_amd.ops import point_decode as point_ops
    monkeypatch.setattr(point_ops, 'NATIVE_POINTS', native)
    head.zero_grad(set_to_none=True)
    leaves = [f.clone().requires_grad_() for f in feats]
    seen = {}
    outs = head(leaves, after_init=seen.update)
    flat = [t for lst in outs for t in lst if t is not None]
    g = pc.gen(9)
    loss = sum((t * torch.randn(tuple(t.shape), generator=g).to(t.device)).sum() for t in flat)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in head.named_parameters() if p.grad is not None}
    grads.update({f'feat{i}': f.grad.detach().clone() for i, f in enumerate(leaves)})
    pre = head.init_stage_targets([tuple(f.shape[-2:]) for f in feats], feats[0], *gt)
    got = {}
    orig = head.get_targets

    def spy(*a, **k):
        got['boxes'] = k['stacked']
        return orig(*a, **k)
    monkeypatch.setattr(head, 'get_targets', spy)
    targets, n_pos = head.refine_stage_targets(pre, seen[head._box_branch()])
    monkeypatch.undo()
    boxes = got['boxes']
    gt_inds = [head.refine_assigner.assign(boxes[i], pre['num_level'], pre['gt_bboxes'][i], None, None).gt_inds
               for i in range(pc.B)]
    torch.cuda.synchronize()
    return [t.detach() for t in flat], boxes, gt_inds, grads, targets, n_pos


@pytest.mark.parametrize('task', TASKS)
def test_head_with_the_switch_on_and_off(task, monkeypatch):
    assert SOFTPLUS_BIT_EQUAL      # (hence torch.equal everywhere below, not a propagated ulp bound)
    head = _head(task)
    feats, gt = _head_inputs(task)
    on = _run_head(head, feats, gt, True, monkeypatch)
    off = _run_head(head, feats, gt, False, monkeypatch)
    assert len(on[0]) == len(off[0]) == len(pc.LEVELS) * (1 + 2 * len(head.branches))
    for i, (a, b) in enumerate(zip(on[0], off[0])):
        assert a.shape == b.shape and torch.equal(a, b), f'output {i}'
    assert torch.equal(on[1], off[1]), 'proposal boxes'
    assert any((a > 0).any() for a in on[2])                   # the assignment is not empty
    for a, b in zip(on[2], off[2]):
        assert a.dtype == torch.long and torch.equal(a, b)     # array_equal
    assert sorted(on[3]) == sorted(off[3]) and len(on[3]) > 20
    for k in on[3]:
        assert torch.equal(on[3][k], off[3][k]), k
    for k in on[4]:
        assert torch.equal(on[4][k], off[4][k]), k
    assert torch.equal(on[5], off[5])


@pytest.mark.parametrize('task', ['bbox', 'pose_bbox'])
def test_head_launches(task, monkeypatch):
    from lsnet_amd import _lib
    from lsnet_amd.ops import point_decode as point_ops
    monkeypatch.setattr(point_ops, 'NATIVE_POINTS', True)
    head = _head(task)
    feats, gt = _head_inputs(task)
    nb = len(head.branches)
    seen = {}

    def logged(fn):
        try:
            _lib.prof_enable(True, ['points'])
            out = fn()
            torch.cuda.synchronize()
            return out, _lib.prof_read()['points']['launches']
        finally:
            _lib.prof_enable(False)
    outs, n_fwd = logged(lambda: head([f.clone().requires_grad_() for f in feats], after_init=seen.update))
    assert n_fwd == 2 * nb                      # one point_decode and one softplus_add per branch
    loss = sum(t.sum() for lst in outs for t in lst if t is not None)
    _, n_bwd = logged(loss.backward)
    assert n_bwd == 2 * nb
    pre = head.init_stage_targets([tuple(f.shape[-2:]) for f in feats], feats[0], *gt)
    _, n_box = logged(lambda: head.refine_stage_targets(pre, seen[head._box_branch()]))
    assert n_box == 1
    monkeypatch.setattr(point_ops, 'NATIVE_POINTS', False)
    _, n_off = logged(lambda: (head(feats), head.refine_stage_targets(pre, seen[head._box_branch()])))
    assert n_off == 0
