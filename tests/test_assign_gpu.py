"""Target assignment as kernels of the library (lsn_centroid_assign / lsn_atss_assign, their batch forms, lsn_dense_targets;
csrc/assign.hip) on the MI355X: against the stored fixture, against the torch statements of core/assigners.py on the device,
inside LSHead.forward_train, and under the no-allocation / graph-capture rules of the training step.  Inputs and their
near-tie condition (checked on the reference side, on the CPU): tests/assign_cases.py."""
import numpy as np
import pytest
import torch

from lsnet_amd import _lib
from lsnet_amd.core import ATSSAssigner, CentroidAssigner, assigners
from lsnet_amd.ops.backend import get_backend
from tests import assign_cases as ac
from tests import golden_cases as gc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _case(case, check=True):
    seed, ng, pseed, _, topks = case
    pts, sizes = ac.grid()
    b, l, e = gu.make_gt(seed, ng, 800, 800)
    props = ac.proposals(pts, pseed)
    if check:
        assert ac.margins_ok(pts, sizes, b, e, props, topks), 'a near-tie in the inputs: replace the case in assign_cases'
    return [t.to(DEV) for t in (pts, b, l, e, props)] + [[s[0] * s[1] for s in sizes]]


def _torch_statement(monkeypatch, fn, *args):
    with monkeypatch.context() as m:
        m.setattr(assigners, 'NATIVE_ASSIGN', False)
        return fn(*args)


def _same(got, want, what):
    assert torch.equal(got.gt_inds, want.gt_inds), what
    assert (got.labels is None) == (want.labels is None) and (got.labels is None or torch.equal(got.labels, want.labels)), what
    if want.max_overlaps is not None:
        pos = want.gt_inds > 0
        assert torch.equal(got.max_overlaps[pos], want.max_overlaps[pos]), what            # the same bits
        assert torch.equal(got.max_overlaps, want.max_overlaps), what                      # and -1e8 elsewhere


def test_entry_points_reproduce_the_fixture():
    """hip_backend's single and batched calls against assign.npz: exact integers, max_overlaps to the fixture's tolerance."""
    ref = gc.load('assign')
    be = get_backend(torch.zeros(1, device=DEV))
    data = [_case(c) for c in ac.CASES[:2]]
    pts, level_len = data[0][0], data[0][5]
    for i, (_, b, l, e, props, _) in enumerate(data):
        gt_inds, labels = be.centroid_assign(pts, b, None, 4.0, 1, l)
        assert np.array_equal(gt_inds.cpu().numpy(), ref[f'init/{i}/gt_inds'])
        assert np.array_equal(labels.cpu().numpy(), ref[f'init/{i}/labels'])
        gt_inds, labels = be.centroid_assign(pts, b, CentroidAssigner.gen_centroid(e, len(b)), 4.0, 3)
        assert labels is None and np.array_equal(gt_inds.cpu().numpy(), ref[f'centroid/{i}/gt_inds'])
        gt_inds, mo, labels = be.atss_assign(props, level_len, b, 9, l)
        assert np.array_equal(gt_inds.cpu().numpy(), ref[f'atss/{i}/gt_inds'])
        gu.check(f'atss/{i}/max_overlaps', mo, ref, gc.FP_TOL, stride=5)
        assert torch.equal(labels, torch.where(gt_inds > 0, l[(gt_inds - 1).clamp(min=0)], -1))
    # both images in one call
    bs, ls, es, ps = ([d[k] for d in data] for k in (1, 2, 3, 4))
    gt_inds, labels = be.centroid_assign_batch(pts, bs, None, 4.0, 1, ls)
    cen, _ = be.centroid_assign_batch(pts, bs, [CentroidAssigner.gen_centroid(e, len(b)) for b, e in zip(bs, es)], 4.0, 3)
    a_inds, a_mo, a_lab = be.atss_assign_batch(torch.stack(ps), level_len, bs, 9, ls)
    for i in range(2):
        assert np.array_equal(gt_inds[i].cpu().numpy(), ref[f'init/{i}/gt_inds'])
        assert np.array_equal(labels[i].cpu().numpy(), ref[f'init/{i}/labels'])
        assert np.array_equal(cen[i].cpu().numpy(), ref[f'centroid/{i}/gt_inds'])
        assert np.array_equal(a_inds[i].cpu().numpy(), ref[f'atss/{i}/gt_inds'])
        gu.check(f'atss/{i}/max_overlaps', a_mo[i], ref, gc.FP_TOL, stride=5)
    # the fixture case of the suite itself, now on the kernels
    assert assigners.NATIVE_ASSIGN
    gc.assign_case(DEV)


@pytest.mark.parametrize('case', ac.CASES + [ac.CROWDED], ids=lambda c: f'gt{c[0]}_G{c[1]}')
def test_native_equals_the_torch_statement(monkeypatch, case):
    """Every seeded image (G = 1 .. 60, and the crowded one: G = 300, which meets the input condition) through the
    assigner classes, native against NATIVE_ASSIGN = False, on the device."""
    pts, b, l, e, props, level_len = _case(case)
    for pos_num, typ in ac.CENTROID_MODES:
        a = CentroidAssigner(scale=4, pos_num=pos_num, iou_type=typ)
        got = a.assign(pts, b, e, None, l)
        _same(got, _torch_statement(monkeypatch, a.assign, pts, b, e, None, l), (pos_num, typ))
        assert (got.gt_inds > 0).any()
    for topk in case[4]:
        a = ATSSAssigner(topk=topk)
        got = a.assign(props, level_len, b, None, l)
        _same(got, _torch_statement(monkeypatch, a.assign, props, level_len, b, None, l), topk)
        assert (got.gt_inds > 0).any()
    # boxes with a score column (ld = 5) and no labels
    props5 = torch.cat([props, torch.rand(len(props), 1, device=DEV)], 1)
    a = ATSSAssigner(topk=9)
    _same(a.assign(props5, level_len, b), _torch_statement(monkeypatch, a.assign, props5, level_len, b), 'ld 5')


def test_constructed_ties_on_the_device(monkeypatch):
    pts, sizes = ac.grid()
    xy = {(int(x), int(y)): i for i, (x, y, s) in enumerate(pts.tolist()) if s == 8}
    pts = pts.to(DEV)
    for name, gts, pos_num, expect in ac.centroid_ties():
        want = torch.zeros(len(pts), dtype=torch.long)
        for p, g in expect.items():
            want[xy[p]] = g
        a = CentroidAssigner(scale=4, pos_num=pos_num, iou_type='center')
        lab = torch.arange(len(gts), device=DEV) + 10
        got = a.assign(pts, gts.to(DEV), None, None, lab)
        assert torch.equal(got.gt_inds.cpu(), want), name
        assert torch.equal(got.labels.cpu(), torch.where(want > 0, want + 9, -1)), name
        _same(got, _torch_statement(monkeypatch, a.assign, pts, gts.to(DEV), None, None, lab), name)
    boxes, level_len, topk, gts, want, iou = ac.atss_tie()
    for order in ([0, 1], [1, 0]):
        a = ATSSAssigner(topk=topk)
        got = a.assign(boxes.to(DEV), level_len, gts[order].to(DEV))
        assert got.gt_inds.tolist() == want and float(got.max_overlaps[2]) == iou
        _same(got, _torch_statement(monkeypatch, a.assign, boxes.to(DEV), level_len, gts[order].to(DEV)), 'atss tie')


def test_filtered_points_and_an_image_without_gts(monkeypatch):
    """The `inside`-filtered case (a padded shape smaller than the grid: shorter levels, the points a subset) through the
    single-image entry points, and a batch whose second image has no gt."""
    pts, b, l, e, props, level_len = _case(ac.CASES[1])
    _, sizes = ac.grid()
    from lsnet_amd.core import PointGenerator
    pg = PointGenerator()
    flags = torch.cat([pg.valid_flags(sz, (min(sz[0], -(-600 // s)), min(sz[1], -(-700 // s))), DEV)
                       for sz, s in zip(sizes, ac.STRIDES)])
    short = [int(f.sum()) for f in torch.split(flags, level_len)]
    assert sum(short) < sum(level_len) and min(short) >= 9
    keep = (b[:, 2] < 700) & (b[:, 3] < 600)
    bb, ll, ee = b[keep], l[keep], e[keep]
    cpu = [t.cpu() for t in (pts[flags], bb, ee, props[flags])]
    assert ac.margins_ok(cpu[0], [(n, 1) for n in short], cpu[1], cpu[2], cpu[3], (9,))
    for pos_num, typ in ac.CENTROID_MODES:
        a = CentroidAssigner(scale=4, pos_num=pos_num, iou_type=typ)
        _same(a.assign(pts[flags], bb, ee, None, ll), _torch_statement(monkeypatch, a.assign, pts[flags], bb, ee, None, ll), typ)
    a = ATSSAssigner(topk=9)
    _same(a.assign(props[flags], short, bb, None, ll), _torch_statement(monkeypatch, a.assign, props[flags], short, bb, None, ll), 'atss')
    # a level shorter than topk keeps the torch path and with it torch's error
    with pytest.raises(RuntimeError):
        a.assign(props[:sum(level_len[:-1]) + 4], level_len[:-1] + [4], b, None, l)

    # batch: image 0 with gts, image 1 without
    init = CentroidAssigner(scale=4, pos_num=1, iou_type='center')
    res = init.assign_batch(pts, [b, b[:0]], [e, e[:0]], [l, l[:0]])
    _same(res[0], _torch_statement(monkeypatch, init.assign, pts, b, e, None, l), 'batch image 0')
    assert res[1].num_gts == 0 and not res[1].gt_inds.any() and (res[1].labels == -1).all()
    res = a.assign_batch(torch.stack([props, props.flip(0)]), level_len, [b, b[:0]], [l, l[:0]])
    _same(res[0], _torch_statement(monkeypatch, a.assign, props, level_len, b, None, l), 'atss batch image 0')
    assert not res[1].gt_inds.any() and (res[1].labels == -1).all() and not res[1].max_overlaps.any()
    assert init.assign_batch(pts, [b[:0], b[:0]], [e[:0], e[:0]]) is None       # nothing to assign: the caller's empty result


@pytest.mark.parametrize('D', [4, 12, 72 + 51])
def test_dense_targets(D):
    g = gu.gen(50 + D)
    G, P = 37, 13343
    table = torch.randn(G, D, generator=g).to(DEV)
    gt_inds = torch.where(torch.rand(P, generator=g) < 0.05, torch.randint(1, G + 1, (P,), generator=g), 0).to(DEV)
    got = get_backend(table).dense_targets(gt_inds, table)
    want = torch.where((gt_inds > 0)[:, None], table[(gt_inds - 1).clamp(min=0)], 0.0)
    assert got.shape == (P, D) and torch.equal(got, want)


@pytest.mark.parametrize('task', ['bbox', 'segm', 'pose_bbox'])
def test_head_losses_are_bit_identical(monkeypatch, task):
    """LSHead.forward_train at the head-fixture shape with the switch on and off: every loss term the same bits."""
    head = gc.build_head(task, DEV, 32)
    head.train()
    boxes, labels, extremes, masks, kps, metas = gc.gt_for(task, DEV)

    def run():
        feats = [f.to(DEV) for f in gu.head_inputs(11, 32)]
        out = head.forward_train(feats, metas, boxes, extremes if task in ('bbox', 'pose_bbox') else None,
                                 [k.clone() for k in kps] if 'pose' in task else None, masks if task == 'segm' else None, labels)
        torch.cuda.synchronize()
        return out
    calls = []
    be = get_backend(boxes[0])
    for name in ('centroid_assign_batch', 'atss_assign_batch', 'dense_targets'):
        monkeypatch.setattr(be, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(be, name), name))
    native = run()
    # one batched call per stage, one gather per image and stage
    assert calls.count('centroid_assign_batch') == 1 and calls.count('atss_assign_batch') == 1, calls
    assert calls.count('dense_targets') == 4, calls
    del calls[:]
    with monkeypatch.context() as m:
        m.setattr(assigners, 'NATIVE_ASSIGN', False)
        plain = run()
    assert not calls
    assert sorted(native) == sorted(plain) and len(native) >= 3
    for k in native:
        assert len(native[k]) == len(plain[k])
        for a, b in zip(native[k], plain[k]):
            assert torch.equal(a, b), (task, k, float(a), float(b))


def test_no_allocation_no_sync_and_graph_replay():
    """After the first call the library allocates nothing and synchronises nowhere (lsn_scratch_stats); a Centroid + ATSS pair
    on preallocated tensors, captured into a single-stream graph, replays to the new gts' assignment after the gt tensors
    were overwritten in place."""
    be = get_backend(torch.zeros(1, device=DEV))
    pts, b0, l0, _, props0, level_len = _case(ac.CASES[1])
    _, b1, l1, _, props1, _ = _case((1777, 12, 2777, None, (9,)), check=False)     # (native against native: no condition needed)
    assert len(b0) == len(b1) == 12
    P = len(pts)
    gt, lab, props = b0.clone(), l0.clone(), props0.clone()
    nb = int(_lib.load().lsn_assign_workspace_bytes(P, 12, 5, 9))
    out_c = (torch.empty((1, P), dtype=torch.long, device=DEV), torch.empty((1, P), dtype=torch.long, device=DEV),
             torch.empty(nb, dtype=torch.uint8, device=DEV))
    out_a = (torch.empty((1, P), dtype=torch.long, device=DEV), torch.empty((1, P), device=DEV),
             torch.empty((1, P), dtype=torch.long, device=DEV), torch.empty(nb, dtype=torch.uint8, device=DEV))

    def pair():
        be.centroid_assign(pts, gt, None, 4.0, 1, lab, out=out_c)
        be.atss_assign(props, level_len, gt, 9, lab, out=out_a)
    pair()
    torch.cuda.synchronize()
    before = _lib.scratch_stats()
    pair()
    be.dense_targets(out_c[0].view(-1), gt)
    torch.cuda.synchronize()
    assert _lib.scratch_stats() == before
    want0 = (out_c[0].clone(), out_a[0].clone(), out_a[1].clone())

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        pair()                                  # warm-up on the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            pair()
    torch.cuda.current_stream().wait_stream(stream)
    gt.copy_(b1), lab.copy_(l1), props.copy_(props1)
    for t in out_c[:2] + out_a[:3]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    c1, _ = be.centroid_assign(pts, b1, None, 4.0, 1, l1)
    a1, m1, _ = be.atss_assign(props1, level_len, b1, 9, l1)
    assert torch.equal(out_c[0].view(-1), c1) and torch.equal(out_a[0].view(-1), a1) and torch.equal(out_a[1].view(-1), m1)
    assert not torch.equal(c1, want0[0].view(-1)) and not torch.equal(a1, want0[1].view(-1))
    gt.copy_(b0), lab.copy_(l0), props.copy_(props0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c[0], want0[0]) and torch.equal(out_a[0], want0[1]) and torch.equal(out_a[1], want0[2])
    assert _lib.scratch_stats() == before
