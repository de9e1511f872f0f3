"""Target assignment of ragged batches on the MI355X: the masked batched calls (lsn_centroid_assign_masked_batch,
lsn_atss_assign_masked_batch) and the per-point targets of a stage (lsn_assign_targets_batch) against the single-image calls
and the torch statements on the FILTERED points, scattered back; inside LSHead.forward_train against the per-image path
(LSNET_NATIVE_RAGGED=0) and the torch statements (LSNET_NATIVE_ASSIGN=0); and under the no-allocation / no-synchronisation /
graph-capture rules of the training step.  Inputs and their near-tie condition: tests/assign_ragged_cases.py (asserted on the
CPU in tests/test_assign_ragged_host.py)."""
import ctypes

import pytest
import torch

from lsnet_amd import _lib
from lsnet_amd.core import ATSSAssigner, CentroidAssigner, assigners
from lsnet_amd.ops.backend import get_backend
from tests import assign_cases as ac
from tests import assign_ragged_cases as rc
from tests import golden_cases as gc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def images():
    """the five images of the table and the one without gts, on the device (built once, read-only)"""
    out = {}
    for k in list(rc.IMAGES) + [None]:
        im = rc.image(k)
        out[k] = {n: (v.to(DEV) if torch.is_tensor(v) else v) for n, v in im.items()}
    return out


@pytest.fixture(scope='module')
def be():
    return get_backend(torch.zeros(1, device=DEV))


def _torch_statement(monkeypatch, fn, *args, **kw):
    with monkeypatch.context() as m:
        m.setattr(assigners, 'NATIVE_ASSIGN', False)
        return fn(*args, **kw)


def _centres(typ, ims):
    if typ != 'centroid':
        return None
    return [CentroidAssigner.gen_centroid(im['extremes'], len(im['boxes'])) if len(im['boxes']) else im['boxes'].new_zeros((0, 2))
            for im in ims]


# ---- 1. entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', rc.BATCHES, ids=lambda b: '_'.join(str(k) for k in b))
def test_masked_batch_equals_single_image_calls_and_torch(monkeypatch, images, be, batch):
    ims = [images[k] for k in batch]
    pts, level_len = ims[0]['pts'], ims[0]['level_len']
    valid = torch.stack([im['flags'] for im in ims])
    gts, labs = [im['boxes'] for im in ims], [im['labels'] for im in ims]
    counts = [im['counts'] for im in ims]
    for pos_num, typ in ac.CENTROID_MODES:
        for with_labels in (True, False):
            gt_inds, labels = be.centroid_assign_batch(pts, gts, _centres(typ, ims), 4.0, pos_num, labs if with_labels else None,
                                                       valid=valid)
            assert (labels is None) == (not with_labels)
            for b, im in enumerate(ims):
                single = rc.centroid_statement(im, pos_num, typ, with_labels)                               # native, filtered
                plain = _torch_statement(monkeypatch, rc.centroid_statement, im, pos_num, typ, with_labels)
                for want in (single, plain):
                    assert torch.equal(gt_inds[b], want[0]), (b, pos_num, typ)
                    assert labels is None or torch.equal(labels[b], want[1]), (b, pos_num, typ)
                assert (gt_inds[b] > 0).any() == (len(im['boxes']) > 0) and not gt_inds[b][~im['flags']].any()
    g = gu.gen(9)
    for ld in (4, 5):
        props = [im['props'] if ld == 4 else torch.cat([im['props'], torch.rand(len(pts), 1, generator=g).to(DEV)], 1) for im in ims]
        for with_labels in (True, False):
            gt_inds, mo, labels = be.atss_assign_batch(torch.stack(props), level_len, gts, rc.TOPK, labs if with_labels else None,
                                                       valid=valid, valid_counts=counts)
            for b, im in enumerate(ims):
                single = rc.atss_statement(im, props[b][:, :4], with_labels)
                plain = _torch_statement(monkeypatch, rc.atss_statement, im, props[b][:, :4], with_labels)
                for want in (single, plain):
                    assert torch.equal(gt_inds[b], want[0]), (b, ld)
                    assert torch.equal(mo[b], want[1]), (b, ld)          # the same bits on positives, -1e8 elsewhere
                    assert labels is None or torch.equal(labels[b], want[2]), (b, ld)
                assert (gt_inds[b] > 0).any() == (len(im['boxes']) > 0)
    # through the assigner classes: AssignResults, and None where a level is short of topk
    res = ATSSAssigner(topk=rc.TOPK).assign_batch(torch.stack([im['props'] for im in ims]), level_len, gts, labs, valid=valid,
                                                  valid_counts=counts)
    assert res is not None and all(torch.equal(r.gt_inds, rc.atss_statement(im)[0]) for r, im in zip(res, ims))
    short = [list(c) for c in counts]
    short[1][-1] = rc.TOPK - 1
    assert ATSSAssigner(topk=rc.TOPK).assign_batch(torch.stack([im['props'] for im in ims]), level_len, gts, labs, valid=valid,
                                                   valid_counts=short) is None
    res = CentroidAssigner(scale=4, pos_num=1, iou_type='center').assign_batch(pts, gts, [im['extremes'] for im in ims], labs,
                                                                              valid=valid)
    assert all(torch.equal(r.gt_inds, rc.centroid_statement(im, 1, 'center')[0]) for r, im in zip(res, ims))


# ---- 2. valid = None ------------------------------------------------------------------------------------------------------
def test_no_mask_and_a_mask_of_ones_give_the_bits_of_the_batched_call(images, be):
    lib = _lib.load()
    ims = [images[0], images[1], images[12]]          # (all their gts, the whole grid: the mask plays no part here)
    pts, level_len, P = ims[0]['pts'], ims[0]['level_len'], len(ims[0]['pts'])
    gts, labs = [im['boxes'] for im in ims], [im['labels'] for im in ims]
    props = torch.stack([im['props'] for im in ims])
    ones = torch.ones((3, P), dtype=torch.bool, device=DEV)
    full = [level_len] * 3
    # today's entry point, called directly
    g, offs, G = be._assign_gts(gts, 'gt_bboxes')
    lab = torch.cat(labs)
    ws = torch.empty(int(lib.lsn_assign_workspace_bytes(3 * P, G, 5, 9)), dtype=torch.uint8, device=DEV)
    c_inds, c_lab = torch.empty((3, P), dtype=torch.long, device=DEV), torch.empty((3, P), dtype=torch.long, device=DEV)
    _lib.check(lib.lsn_centroid_assign_batch(_lib.ptr(pts), P, _lib.ptr(g), None, 3, offs, 4.0, 3, _lib.ptr(lab), _lib.ptr(c_inds),
                                             _lib.ptr(c_lab), _lib.ptr(ws), _lib.stream()))
    a_inds, a_lab = torch.empty((3, P), dtype=torch.long, device=DEV), torch.empty((3, P), dtype=torch.long, device=DEV)
    a_mo = torch.empty((3, P), device=DEV)
    lens = (ctypes.c_int * 5)(*level_len)
    _lib.check(lib.lsn_atss_assign_batch(_lib.ptr(props), 4, P, 5, lens, _lib.ptr(g), 3, offs, 9, _lib.ptr(lab), _lib.ptr(a_inds),
                                         _lib.ptr(a_mo), _lib.ptr(a_lab), _lib.ptr(ws), _lib.stream()))
    torch.cuda.synchronize()
    for valid, vc in ((None, None), (ones, full), (ones.view(torch.uint8), full)):
        gi, l = be.centroid_assign_batch(pts, gts, None, 4.0, 3, labs, valid=valid)
        assert torch.equal(gi, c_inds) and torch.equal(l, c_lab)
        gi, mo, l = be.atss_assign_batch(props, level_len, gts, 9, labs, valid=valid, valid_counts=vc)
        assert torch.equal(gi, a_inds) and torch.equal(l, a_lab) and torch.equal(mo, a_mo)
    assert (c_inds > 0).any() and (a_inds > 0).any()


# ---- 3. a tie across the mask -----------------------------------------------------------------------------------------------
def test_a_tie_across_the_mask(monkeypatch, be):
    pts, _ = ac.grid()
    xy = {(int(x), int(y)): i for i, (x, y, s) in enumerate(pts.tolist()) if s == 8}
    name, gts, _, _ = ac.centroid_ties()[0]
    assert name == 'four_equal_k1'
    pts, gts = pts.to(DEV), gts.to(DEV)
    flags = torch.ones(len(pts), dtype=torch.bool, device=DEV)
    flags[xy[(96, 96)]] = False
    for pos_num, expect in ((1, [(104, 96)]), (3, [(104, 96), (96, 104), (104, 104)])):
        want = torch.zeros(len(pts), dtype=torch.long, device=DEV)
        want[[xy[p] for p in expect]] = 1
        gt_inds, _ = be.centroid_assign_batch(pts, [gts], None, 4.0, pos_num, valid=flags[None])
        assert torch.equal(gt_inds[0], want), pos_num
        a = CentroidAssigner(scale=4, pos_num=pos_num, iou_type='center')
        ref = _torch_statement(monkeypatch, a.assign, pts[flags], gts, None)
        assert torch.equal(rc.scatter(flags, ref.gt_inds, 0), want), pos_num


# ---- 4. the per-point targets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [4, 12, 72 + 51])
@pytest.mark.parametrize('with_labels', [True, False])
def test_assign_targets_batch(images, be, D, with_labels):
    batch = [images[0], images[12], images[None]]
    background = 80
    g = gu.gen(60 + D)
    tables = [torch.randn(len(im['boxes']), D, generator=g).to(DEV) for im in batch]
    labs = [torch.randint(0, 80, (len(im['boxes']),), generator=g).to(DEV) for im in batch]
    gt_inds = torch.stack([rc.seeded_gt_inds(70 + i, im['flags'].cpu(), len(im['boxes'])) for i, im in enumerate(batch)]).to(DEV)
    for valid in (torch.stack([im['flags'] for im in batch]), None):
        got = be.assign_targets_batch(gt_inds, valid, tables, labs if with_labels else None, background)
        assert torch.equal(got[4], (gt_inds > 0).sum(1)) and got[4][0] > 0 and got[4][1] > 0 and got[4][2] == 0
        for b, im in enumerate(batch):
            flags = im['flags'] if valid is not None else torch.ones_like(im['flags'])
            want = rc.targets_statement(gt_inds[b], flags, tables[b], labs[b] if with_labels else None, background)
            for a, w in zip(got[:4], want[:4]):
                assert a[b].dtype == w.dtype and torch.equal(a[b], w), (b, D)
            assert got[4][b] == want[4]


# ---- 5. the head ------------------------------------------------------------------------------------------------------------
def _ragged_inputs(task, empty_second):
    boxes, labels, ext, metas, _, _ = gu.edge_case_targets('ragged')
    if empty_second:
        boxes, labels, ext = [boxes[0], boxes[1][:0]], [labels[0], labels[1][:0]], [ext[0], ext[1][:0]]
    masks = [gu.make_polygons(b) for b in boxes]
    kps = [gu.make_keypoints(200 + i, b) if len(b) else torch.zeros(0, 51) for i, b in enumerate(boxes)]
    to = lambda lst: [t.to(DEV) for t in lst]           # noqa: E731
    return to(boxes), to(labels), to(ext), masks, to(kps), metas


def _wrap(monkeypatch, be, calls, seen=None):
    for name in ('centroid_assign_batch', 'atss_assign_batch', 'assign_targets_batch', 'dense_targets'):
        def make(f, n):
            def wrapped(*a, **k):
                calls.append(n)
                if seen is not None and not seen and n == 'atss_assign_batch':      # (the first call's inputs)
                    seen.append((a[0].detach().cpu(), [g.cpu() for g in a[2]]))
                return f(*a, **k)
            return wrapped
        monkeypatch.setattr(be, name, make(getattr(be, name), name))


# (the second image emptied of gts runs for bbox: the ground-truth preparation of segm / pose raises for an image without
# instances, as the reference's does -- tests/test_live_reference.py::test_image_without_instances_raises_as_reference --
# and nothing reaches the assignment)
@pytest.mark.parametrize('task,empty_second', [('bbox', False), ('segm', False), ('pose_bbox', False), ('bbox', True)],
                         ids=['bbox', 'segm', 'pose_bbox', 'bbox_second_image_empty'])
def test_head_losses_on_a_ragged_batch(monkeypatch, be, task, empty_second):
    """LSHead.forward_train on the ragged batch of golden_util.edge_case_targets: the batched path gives the bits of the
    per-image path and of the torch statements, in one assign call per stage and one target call per stage."""
    head = gc.build_head(task, DEV, 32)
    head.train()
    inputs = _ragged_inputs(task, empty_second)
    feats = [f.to(DEV) for f in gu.head_inputs(11, 32)]

    def run(backward=False):
        leaves = [f.clone().requires_grad_() for f in feats]
        out = head.forward_train(leaves, *_head_args(task, inputs))
        if backward:
            sum(sum(v) if isinstance(v, (list, tuple)) else v.sum() for v in out.values()).backward()
            assert all(f.grad is not None and torch.isfinite(f.grad).all() for f in leaves)
        torch.cuda.synchronize()
        return out
    calls, seen = [], []
    _wrap(monkeypatch, be, calls, seen)
    native = run(backward=True)
    assert calls.count('centroid_assign_batch') == 1 and calls.count('atss_assign_batch') == 1, calls
    assert calls.count('assign_targets_batch') == 2 and calls.count('dense_targets') == 0, calls
    # the condition under which the kernels and the torch statements must agree: no refine-stage candidate within 1e-5 of its
    # gt's threshold, on the reference side
    (boxes_cpu, gts_cpu), = seen
    valid, counts = head.get_valid([tuple(f.shape[-2:]) for f in feats], inputs[5], DEV)
    for b in range(2):
        if len(gts_cpu[b]):
            f = valid[b].cpu()
            assert ac.atss_margin(boxes_cpu[b][f][:, :4], counts[b], gts_cpu[b], 9) > 1e-5, 'a near-tie: change the gt seed'
    del calls[:]
    with monkeypatch.context() as m:
        m.setattr(assigners, 'NATIVE_RAGGED', False)
        per_image = run()
    assert calls.count('assign_targets_batch') == 0 and calls.count('dense_targets') == 4 - 2 * empty_second, calls
    del calls[:]
    with monkeypatch.context() as m:
        m.setattr(assigners, 'NATIVE_ASSIGN', False)
        plain = run()
    assert not calls
    assert sorted(native) == sorted(per_image) == sorted(plain) and len(native) >= 3
    for k in native:
        assert len(native[k]) == len(per_image[k]) == len(plain[k])
        for a, b, c in zip(native[k], per_image[k], plain[k]):
            assert torch.isfinite(a) and torch.equal(a, b), (task, k, float(a), float(b))
            assert torch.equal(a, c), (task, k, float(a), float(c))
    if task == 'bbox':      # the step reads nothing back: no boolean index, no int(tensor)
        leaves = [f.clone().requires_grad_() for f in feats]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            out = head.forward_train(leaves, *_head_args(task, inputs))
        finally:
            torch.cuda.set_sync_debug_mode('default')
        for k in native:
            assert all(torch.equal(a, b) for a, b in zip(out[k], native[k])), k


def _head_args(task, inputs):
    boxes, labels, ext, masks, kps, metas = inputs
    return (metas, boxes, ext if task in ('bbox', 'pose_bbox') else None, [k.clone() for k in kps] if 'pose' in task else None,
            masks if task == 'segm' else None, labels)


# ---- 6. a level short of topk -------------------------------------------------------------------------------------------------
def test_short_level_raises_as_before(monkeypatch):
    """pad_shape (128, 160): the stride-128 level keeps 1 x 2 cells.  ATSS' batched call declines, the per-image path runs and
    torch.topk raises -- the same exception type with the switch on and off."""
    head = gc.build_head('bbox', DEV, 32)
    head.train()
    inputs = list(_ragged_inputs('bbox', False))
    inputs[5] = [inputs[5][0], dict(inputs[5][1], pad_shape=(128, 160, 3), img_shape=(128, 160, 3))]
    feats = [f.to(DEV) for f in gu.head_inputs(11, 32)]
    assert head.get_valid([tuple(f.shape[-2:]) for f in feats], inputs[5], DEV)[1][1][-1] == 2
    raised = []
    for switch in (True, False):
        with monkeypatch.context() as m:
            m.setattr(assigners, 'NATIVE_RAGGED', switch)
            with pytest.raises(Exception) as info:
                head.forward_train(feats, *_head_args('bbox', inputs))
            torch.cuda.synchronize()
            raised.append(info.type)
    assert raised[0] is raised[1] and issubclass(raised[0], RuntimeError), raised


# ---- 7. library hygiene -------------------------------------------------------------------------------------------------------
def test_no_allocation_and_graph_replay_with_a_mask(images, be):
    """After a first call a masked Centroid + ATSS + targets triple on preallocated outputs leaves lsn_scratch_stats alone;
    captured into a single-stream graph it replays to the new assignment after gts AND mask were overwritten in place."""
    a, b = images[1], images[12]
    pts, level_len, P = a['pts'], a['level_len'], len(a['pts'])
    n = len(a['boxes'])
    assert n <= len(b['boxes'])
    gt, lab, props = a['boxes'].clone(), a['labels'].clone(), a['props'].clone()
    valid = a['flags'].clone()[None]
    counts = [[min(x, y) for x, y in zip(a['counts'], b['counts'])]]       # host integers, the same for both states
    nb = int(_lib.load().lsn_assign_workspace_bytes(P, n, 5, 9))
    long = lambda *s: torch.empty(s, dtype=torch.long, device=DEV)          # noqa: E731
    out_c = (long(1, P), long(1, P), torch.empty(nb, dtype=torch.uint8, device=DEV))
    out_a = (long(1, P), torch.empty((1, P), device=DEV), long(1, P), torch.empty(nb, dtype=torch.uint8, device=DEV))
    out_t = (torch.empty((1, P, 4), device=DEV), long(1, P), torch.empty((1, P), device=DEV), torch.empty((1, P, 4), device=DEV),
             long(1))

    def triple():
        be.centroid_assign_batch(pts, [gt], None, 4.0, 1, [lab], valid=valid, out=out_c)
        be.atss_assign_batch(props[None], level_len, [gt], 9, [lab], valid=valid, valid_counts=counts, out=out_a)
        be.assign_targets_batch(out_a[0], valid, [gt], [lab], 80, out=out_t)
    triple()
    torch.cuda.synchronize()
    before = _lib.scratch_stats()
    triple()
    torch.cuda.synchronize()
    assert _lib.scratch_stats() == before
    outs = out_c[:2] + out_a[:3] + out_t
    want0 = [t.clone() for t in outs]

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        triple()                                # warm-up on the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            triple()
    torch.cuda.current_stream().wait_stream(stream)
    gt.copy_(b['boxes'][:n]), lab.copy_(b['labels'][:n]), props.copy_(b['props']), valid.copy_(b['flags'][None])
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    c1 = be.centroid_assign_batch(pts, [b['boxes'][:n]], None, 4.0, 1, [b['labels'][:n]], valid=b['flags'][None])
    a1 = be.atss_assign_batch(b['props'][None], level_len, [b['boxes'][:n]], 9, [b['labels'][:n]], valid=b['flags'][None],
                              valid_counts=counts)
    t1 = be.assign_targets_batch(a1[0], b['flags'][None], [b['boxes'][:n]], [b['labels'][:n]], 80)
    for got, want in zip(outs, list(c1) + list(a1) + list(t1)):
        assert torch.equal(got, want)
    assert not torch.equal(c1[0], want0[0]) and not torch.equal(a1[0], want0[2]) and not torch.equal(t1[2], want0[7])
    assert not out_a[0][0][~b['flags']].any() and (out_t[2][0] == b['flags'].float()).all()       # the NEW mask was read
    gt.copy_(a['boxes']), lab.copy_(a['labels']), props.copy_(a['props']), valid.copy_(a['flags'][None])
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, want0):
        assert torch.equal(got, want)
    assert _lib.scratch_stats() == before
